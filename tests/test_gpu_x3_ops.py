"""The split-operand GEMMs (dcpt_amd/csrc/gemm_x3.hip, the opt-in precision mode "bf16x3") per epilogue, operand form and ragged extent.

tests/test_gpu_x3.py holds the mode to float64 for A_PLAIN / E_PLAIN forward at M >= 24 800 alone; everything else reaches it through the
second pass of tests/conftest.py at fp32 tolerances of 2e-5 .. 1e-4, which a dropped piece product (about 2^-17 per product) passes.  Here
every public op that can launch the mode runs at the SMALLEST shape at which each form can still go wrong -- first with the exact
fp32-MFMA kernels, then with the mode forced onto every eligible launch (min_tiles = 1) on the same inputs -- under the red zone
(tests/redzone.py) and with the launch trace (tests/kernel_trace.py) asserting the exact count of nt_f32.x3 / tn_f32.x3 launches and of
every fp32 family that remains (hard-coded beside the list of the op's GEMMs: an eligibility edit fails the test instead of re-routing it).

Three kinds of assertion:
  a  the run in the mode against the float64 restatement of the op's own test module, at that module's fp32 tolerances;
  b  rms and max error against float64 of the run in the mode NOT ABOVE the fp32-MFMA run's on the same inputs, for every tensor a launch
     in the mode writes (outputs, input gradients, the gradients of the 1 x 1 weights and their biases / gains): the criterion of
     tests/test_gpu_x3.py, rms <= 1.1 x and max <= 1.25 x the fp32 kernel's, widened only by the margin measured below;
  c  conv_nobias on small-integer operands whose every partial sum is an integer below 2^24 (asserted on the float64 product of the
     absolute values): each piece product and each fp32 accumulation is then exact and y, dx, dw must be BIT-EQUAL to float64.
Kinds a and b run twice: on uniform [-1, 1) inputs and on an adversarial pass -- every pixel row of an activation (input and output
gradient) scaled by 2^u, every row of a 1 x 1 weight by 2^v, the low 16 mantissa bits of all of them redrawn non-zero so that the second and
third bf16 piece of every operand are populated.  u, v are drawn from {-12..12}; in the TransformerBlock v is drawn from {-8..8}: with
one head the gradient of ``temperature`` is ONE scalar, a sum of cancelling terms, and with weight rows at 2^+-12 plain fp32 arithmetic (the
oracle evaluated in float32 against itself in float64, five seeds, dim 256) misses the module's 3e-4 on it in three seeds of five (4.0e-3,
3.8e-4, 3.2e-3), so the fp32-MFMA run could not be held to kind a either; at 2^+-8 the same measurement gives 2.4e-5 at most.

(operand form, epilogue / TN)                      -> case that proves by its trace count that it ran in the mode
  A_PLAIN  E_PLAIN                                    test_conv_nobias (forward, dx), test_nafblock (B3, B11; B6 at P = 35, 72)
  A_PLAIN  E_BIAS                                     test_nafblock (conv1), test_nafblock_local (conv1)
  A_SCALE  E_RESID  (split3 with kscale, per image)   test_nafblock (conv3: nimg = 2, 3, 1)
  A_PLAIN  E_RESID                                    test_nafblock (conv5), test_nafblock_local (conv3, conv5), test_transformer_block (proj)
  A_PLAIN  E_BIASGATE                                 test_nafblock (conv4), test_nafblock_local (conv4)
  A_PLAIN  E_SGBWD                                    test_nafblock (B1)
  A_PLAIN  E_DOTCOL                                   test_nafblock (2, 256, 16, 8) (B6, P = 128)
  A_PLAIN  E_MUL                                      test_nafblock_local (smap GEMM)
  A_PLAIN  E_ADDSCALED, batched, cscale strides       test_transformer_block (MDTA backward dq, dk)
  A_PLAIN  E_PLAIN batched (nb1 * nb2 = 4 and 2)      test_transformer_block (attn @ v twice, dv: one split image per problem)
  TN, plain, ragged splits                            test_conv_nobias Ci = 256 / 1024: M = 600 -> 224 / 224 / 152 rows, M = 257 -> 160 / 97,
                                                      M = 255 and M = 64 -> one split (M = 63 and M = 1: fp32, X3_TN_MIN_ROWS)
  TN with column sums, one and two tiles along K      test_nafblock C = 256 (tilesK = 1) and C = 512 (tilesK = 2); image-aligned splits of
                                                      128 rows at (2, 256, 16, 8)

The margin of kind b.  At a few hundred to a few thousand elements the ratio of two kernels' errors is noisy, and on the adversarial pass a
handful of rows carries the whole error.  The fp32-MFMA kernel's OWN error against float64 was therefore measured over five input seeds
per case and tensor (the reference, not the code under test; seed 0 is the test's input); MARGIN holds, per family of cases and pass, the
largest max / min over the seeds of that error -- of its rms for the rms criterion, of its max for the max criterion -- where that exceeds
1.1 / 1.25.  Measured on an MI355X (beside it: the largest bf16x3 / fp32-MFMA ratio over the same seeds, which the margin was NOT fitted to):
                               fp32-MFMA error, max / min over 5 seeds      bf16x3 / fp32-MFMA, largest of 5 seeds
    family, pass                      rms       max                             rms       max
    conv M <= 64   uniform            1.30      2.27                            1.08      1.69
    conv M <= 64   adversarial        2.26      4.22                            1.53      2.93
    conv M >= 255  uniform            1.02      1.76                            0.86      1.38
    conv M >= 255  adversarial        1.64      2.75                            1.07      1.63
    nafblock       uniform            1.44      4.45  (bias gradients, 256..1024 elements)   1.17      1.79
    nafblock       adversarial        8.63     22.41                            3.31      3.26
    nafblock_local uniform            1.10      1.80                            0.92      1.14
    nafblock_local adversarial        1.50      2.49                            1.02      1.44
    transformer    uniform            1.28      2.37                            1.24      1.56
    transformer    adversarial        5.92      7.40                            2.34      3.86
On uniform inputs the rms error of the mode is 0.81 - 0.86 of the fp32-MFMA kernel's in every conv_nobias tensor from 64 terms of reduction
on (K = 64 .. 1024, M = 64 .. 600) and 0.85 - 1.00 in the blocks' y and dx.  A dropped piece product of the third order costs ~2^-17 of a product, 5 - 25 times the fp32 kernel's error here: above every
margin of the uniform pass and of kind c; the adversarial margins of the blocks (8.6 / 22) would let it pass, that pass is there for kind a
and for gross errors of scale.
"""
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import keyed_tensor
from kernel_trace import kernel_trace
from oracle import nafnet_oracle as O
from oracle import promptir_oracle as PO
from oracle import restormer_oracle as R
from redzone import redzone
from tests import test_gpu_parity as TPA
from tests import test_gpu_promptir as TPR
from tests import test_gpu_restormer as TRS
from tests import test_gpu_tlsc_bf16 as TTL
from tests.test_gpu_gemm_tiles import Report, assert_gemms, f64, rand

pytestmark = pytest.mark.gpu

# kind b: (rms, max) factors on the fp32-MFMA kernel's error -- the criterion of tests/test_gpu_x3.py unless the module docstring says why not
MARGIN = {("conv M<=64", "uniform"): (1.30, 2.27), ("conv M<=64", "adversarial"): (2.26, 4.22),
          ("conv", "uniform"): (1.1, 1.76), ("conv", "adversarial"): (1.64, 2.75),
          ("nafblock", "uniform"): (1.44, 4.45), ("nafblock", "adversarial"): (8.63, 22.41),
          ("local", "uniform"): (1.1, 1.80), ("local", "adversarial"): (1.50, 2.49),
          ("transformer", "uniform"): (1.28, 2.37), ("transformer", "adversarial"): (5.92, 7.40)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


class _Switch:
    def __init__(self, dev):
        self.dev = dev

    def on(self):
        from dcpt_amd import functional as DF

        DF.set_gemm_precision("bf16x3", device=self.dev, min_tiles=1)

    def off(self):
        from dcpt_amd import functional as DF

        DF.set_gemm_precision("fp32")


@pytest.fixture()
def x3(dev):
    from dcpt_amd import functional as DF

    misses = DF.gemm_x3_scratch_misses()
    yield _Switch(dev)
    DF.set_gemm_precision("fp32")
    assert DF.gemm_x3_scratch_misses() == misses, "a launch fell back to the fp32 kernels: the split-image scratch is too small"


def both_modes(x3, op, nt, tn):
    """``op()`` (forward + backward on fresh leaves, returns {name: tensor}) with the fp32-MFMA kernels, then in the mode: both under the
    red zone, the first with no launch in the mode, the second with exactly the launches ``nt`` / ``tn``"""
    x3.off()
    with redzone() as rz, kernel_trace() as tr:
        o32 = op()
    assert rz.count > 0
    tr.assert_not_ran("nt_f32.x3", "tn_f32.x3")
    x3.on()
    try:
        with redzone() as rz, kernel_trace() as tr:
            o3 = op()
    finally:
        x3.off()
    assert rz.count > 0
    assert_gemms(tr, nt, tn)
    return o32, o3


def err2(a, ref):
    """(rms error / rms of the reference, max error / max of the reference): the two figures of tests/test_gpu_x3.py"""
    d = a.detach().double() - ref
    return float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), float(d.abs().max() / ref.abs().max())


class Ratio:
    """kind b: every figure printed before anything is asserted; the case fails at the end with every miss"""

    def __init__(self, label, family, pass_):
        self.label, self.margin, self.fail, self.figs = label, MARGIN[(family, pass_)], [], {}

    def cmp(self, name, a32, a3, ref):
        ref = ref.detach()
        (r32, m32), (r3, m3) = err2(a32, ref), err2(a3, ref)
        self.figs[name] = (r32, m32, r3, m3)
        print(f"[x3] {self.label} {name}: rms error fp32-MFMA {r32:.2e} / bf16x3 {r3:.2e} (x {r3 / max(r32, 1e-300):.2f}); "
              f"max {m32:.2e} / {m3:.2e} (x {m3 / max(m32, 1e-300):.2f})")
        if not (r3 <= self.margin[0] * r32 and m3 <= self.margin[1] * m32):   # (a NaN fails)
            self.fail.append(f"{name}: bf16x3 rms {r3:.3e} / max {m3:.3e} against fp32-MFMA {r32:.3e} / {m32:.3e}: above "
                             f"{self.margin[0]} x / {self.margin[1]} x")

    def worst(self):
        tiny = 1e-300
        return max(f[2] / max(f[0], tiny) for f in self.figs.values()), max(f[3] / max(f[1], tiny) for f in self.figs.values())

    def done(self):
        print(f"[x3] {self.label}: worst bf16x3 / fp32-MFMA error ratio rms {self.worst()[0]:.2f}, max {self.worst()[1]:.2f}")
        assert not self.fail, f"{self.label}: {len(self.fail)} error comparison(s) missed:\n" + "\n".join(self.fail)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def low_bits(t, seed):
    """the low 16 mantissa bits of every element redrawn from 1 .. 65535: the second and third bf16 piece of the value are non-zero"""
    g = torch.Generator(device=t.device).manual_seed(seed)
    low = torch.randint(1, 1 << 16, t.shape, generator=g, device=t.device, dtype=torch.int32)
    return ((t.view(torch.int32) & -65536) | low).view(torch.float32)


def pow2(dev, shape, span, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.exp2(torch.randint(-span, span + 1, shape, generator=g, device=dev).float())


def adversarial_map(x, seed, span=12):
    """every pixel row of an NHWC map times 2^u, u from {-span..span}; low mantissa bits non-zero"""
    B, _, H, W = x.shape
    return low_bits(x * pow2(x.device, (B, 1, H, W), span, seed), seed + 1).contiguous(memory_format=torch.channels_last)


def adversarial_weight(w, seed, span):
    """every row of a 1 x 1 conv weight [N][K][1][1] times 2^v, v from {-span..span}; low mantissa bits non-zero"""
    return low_bits((w * pow2(w.device, (w.shape[0], 1, 1, 1), span, seed)).contiguous(), seed + 1).contiguous()


def is_gemm_weight(k, v):
    return v.dim() == 4 and v.shape[1] > 1 and v.shape[2] == 1 and v.shape[3] == 1 and k.endswith("weight")


def block_inputs(dev, shape, P, pass_, seed, vspan=12):
    """(x, output gradient, parameters) of a block case: uniform [-1, 1) maps and the keyed parameters, or their adversarial pass (every
    1 x 1 conv weight of the block is a GEMM's weight operand)"""
    x, go = rand(dev, shape, 100 + 10 * seed), rand(dev, shape, 101 + 10 * seed)
    if pass_ == "adversarial":
        x, go = adversarial_map(x, 102 + 10 * seed), adversarial_map(go, 104 + 10 * seed)
        P = {k: adversarial_weight(v, 200 + 10 * seed + i, vspan) if is_gemm_weight(k, v) else v for i, (k, v) in enumerate(P.items())}
    return x, go, P


PASSES = ["uniform", "adversarial"]


# ---- 1. conv_nobias, 1 x 1 (dchead.hip conv_fwd / conv_bwd) ----------------------------------------------------------------------------
# forward  A_PLAIN/E_PLAIN (M, Co; K = Ci) | dx  A_PLAIN/E_PLAIN (M, Ci; K = Co) | dw  TN plain, no column sums (Co, Ci)
# The mode takes an NT launch iff N % 256 == 0 and K % 64 == 0, a TN launch iff N % 256 == 0 and K % 256 == 0 (gemm_nt_x3_ok, gemm_tn_x3_ok):
#   Ci = 64          forward in the mode (one pair of k-tiles of 32);  dx N = 64: fp32 128 x 64;  dw K = 64: fp32 128 x 64
#   Ci = 192         forward in the mode (three pairs);  dx N = 192, a handful of tiles: fp32 128 x 64;  dw K = 192 pads least on 128 x 96
#   Ci = 256, 1024   forward, dx (K = Co = 256 / 512) and dw in the mode (1024: 16 pairs, the ring of k-tiles wraps many times)
# and a TN launch needs M >= 64 (X3_TN_MIN_ROWS: below, the dropped piece products stand above the fp32 kernel's own error; at M = 1, one
# product per element, the mode measured rms 5.7e-8 / max 1.3e-7 against float64 where the fp32 kernel has 2.5e-8 / 3.0e-8).
# split plan of the TN launches in the mode (gemm_tn_x3_plan: want = min(256 / tiles, cdiv(M, 256)), rows_per_split = cdiv(cdiv(M, want), 32) * 32,
# splits = cdiv(M, rows_per_split); tiles = (Co / 256) * (Ci / 256) <= 8, so want = cdiv(M, 256) at every M here):
#   M = 600: want 3, rows_per_split 224, splits of 224 / 224 / 152 rows (the last shorter and no multiple of 32: ten pixel steps of 16, the last of 8)
#   M = 257: want 2, rows_per_split 160, splits of 160 / 97;   M = 255: one split of 255 (rows_per_split 256);   M = 64: one split, rows_per_split 64
#   M = 63, M = 1: the fp32 kernel (plain, no column sums, N and K multiples of 128: 128 x 128 tiles)
CONV_NT = {64: {"x3": 1, "128x64": 1}, 192: {"x3": 1, "128x64": 1}, 256: {"x3": 2}, 1024: {"x3": 2}}
CONV_TN = {64: {"128x64": 1}, 192: {"128x96": 1}, 256: {"x3": 1}, 1024: {"x3": 1}}
CONV_TN_SHORT = {"128x128": 1}   # Ci = 256, 1024 at M < 64
CONV_SHAPES = [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 15, 17), (1, 257, 1), (3, 10, 20)]   # M = 1, 63, 64 (both sides of X3_TN_MIN_ROWS), 255, 257, 600
CONV_WIDTHS = [(Ci, Co) for Ci in (64, 192, 256, 1024) for Co in (256, 512)]


def tn_in_mode(Ci, M):
    return Ci % 256 == 0 and M >= 64


def conv_run(x3, x, w, go, Ci):
    from dcpt_amd import functional as DF

    M = x.shape[0] * x.shape[2] * x.shape[3]

    def op():
        xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = DF.conv_nobias(xg, wg)
        y.backward(go)
        return {"y": y.detach(), "dx": xg.grad, "dw": wg.grad}

    return both_modes(x3, op, CONV_NT[Ci], CONV_TN_SHORT if Ci % 256 == 0 and not tn_in_mode(Ci, M) else CONV_TN[Ci])


def conv_case(dev, x3, Ci, Co, shape, pass_, seed=0):
    B, H, W = shape
    M = B * H * W
    x, go = rand(dev, (B, Ci, H, W), 1 + 10 * seed), rand(dev, (B, Co, H, W), 2 + 10 * seed)
    g = torch.Generator(device=dev).manual_seed(3 + 10 * seed)
    w = (torch.rand((Co, Ci, 1, 1), generator=g, device=dev) * 2 - 1) / Ci ** 0.5
    if pass_ == "adversarial":
        x, go, w = adversarial_map(x, 4 + 10 * seed), adversarial_map(go, 6 + 10 * seed), adversarial_weight(w, 8 + 10 * seed, 12)
    xr, wr = f64(x), f64(w)
    yr = F.conv2d(xr, wr)   # (tests/test_gpu_restormer.py test_helpers: the op's own restatement, here in float64 on the device)
    yr.backward(go.double())
    ref = {"y": yr, "dx": xr.grad, "dw": wr.grad}
    o32, o3 = conv_run(x3, x, w, go, Ci)
    label = f"conv_nobias {Ci}->{Co} M={M} {pass_}"
    rep, rat = Report(TRS, label), Ratio(label, "conv M<=64" if M <= 64 else "conv", pass_)
    in_mode = ["y"] + (["dx"] if Ci % 256 == 0 else []) + (["dw"] if tn_in_mode(Ci, M) else [])
    for n in ("y", "dx", "dw"):
        rep.cmp(n, o3[n], ref[n], 1e-5)
        if n in in_mode:
            rat.cmp(n, o32[n], o3[n], ref[n])
    return rep, rat


@pytest.mark.parametrize("Ci,Co", CONV_WIDTHS)
def test_conv_nobias(dev, x3, Ci, Co):
    done = [r for shape in CONV_SHAPES for pass_ in PASSES for r in conv_case(dev, x3, Ci, Co, shape, pass_)]
    for r in done:
        r.done()


# Kind c.  ``wide``: odd integers of 17-18 significant bits (all three bf16 pieces non-zero); ``mid``: odd integers of ``bits`` bits (two pieces);
# ``small``: {-2..2}.  A matrix keeps ``nz`` non-zero elements per row (or per column), at random places, so that every sum of absolute
# products stays below 2^24 while every k, every row and every column is covered by some non-zero product.
def _sparse(vals, nz, dim, g):
    if nz >= vals.shape[dim]:
        return vals
    rank = torch.rand(vals.shape, generator=g, device=vals.device).argsort(dim).argsort(dim)
    return vals * (rank < nz)


def _ints(dev, shape, lo_bits, hi_bits, g):
    mag = torch.randint(1 << (lo_bits - 1), 1 << hi_bits, shape, generator=g, device=dev) | 1
    sign = torch.randint(0, 2, shape, generator=g, device=dev) * 2 - 1
    return (mag * sign).double()


def _small(dev, shape, g):
    return torch.randint(-2, 3, shape, generator=g, device=dev).double()


def exact_operands(dev, pattern, M, Ci, Co, seed):
    """float64 integer matrices x [M][Ci], w [Co][Ci], dy [M][Co] of one value pattern; the bound on every partial sum is asserted by the caller"""
    g = torch.Generator(device=dev).manual_seed(seed)
    if pattern == "wide activations":     # x: three pieces, w and dy in plane 0 only;  |x w| < 2^19 a product: 32 per row;  dw: 32 per column of dy
        x = _sparse(_ints(dev, (M, Ci), 17, 18, g), 32, 1, g)
        w = _small(dev, (Co, Ci), g)
        dy = _sparse(_small(dev, (M, Co), g), 32, 0, g)
    elif pattern == "wide weights":       # the transpose: planes 1 and 2 of split3_kernel;  y: 32 per row of x;  dx: 32 per row of dy
        x = _sparse(_small(dev, (M, Ci), g), 32, 1, g)
        w = _ints(dev, (Co, Ci), 17, 18, g)
        dy = _sparse(_small(dev, (M, Co), g), 32, 1, g)
    else:                                 # "both mid": x 12 bits, w 9-10, dy 9: |x w| < 2^22: 4 per row of x;  |dy w| < 2^19: 4 per row of dy;
        x = _sparse(_ints(dev, (M, Ci), 12, 12, g), 4, 1, g)    # |dy x| < 2^21: a pair (co, ci) may meet in 8 pixels (it does in 0.6 at most
        w = _ints(dev, (Co, Ci), 9, 10, g)                     # on average); the caller asserts the bound
        dy = _sparse(_ints(dev, (M, Co), 9, 9, g), 4, 1, g)
    return x, w, dy


EXACT_PATTERNS = ["wide activations", "wide weights", "both mid"]


@pytest.mark.parametrize("Ci,Co", CONV_WIDTHS)
def test_conv_nobias_exact_on_integers(dev, x3, Ci, Co):
    """kind c: y, dx and dw of the run in the mode bit-equal to the float64 result, three value patterns, every M of CONV_SHAPES"""
    fail = []
    for shape in CONV_SHAPES:
        B, H, W = shape
        M = B * H * W
        for i, pattern in enumerate(EXACT_PATTERNS):
            x, w, dy = exact_operands(dev, pattern, M, Ci, Co, 1000 * i + M)
            bound = max(float((x.abs() @ w.abs().t()).max()), float((dy.abs() @ w.abs()).max()), float((dy.abs().t() @ x.abs()).max()))
            assert bound <= 2 ** 24, f"{pattern} M={M}: a partial sum may reach {bound:.0f} > 2^24: the inputs do not make the arithmetic exact"
            ref = {"y": x @ w.t(), "dx": dy @ w, "dw": dy.t() @ x}
            assert all(float(r.abs().max()) > 0 for r in ref.values())
            nchw = lambda t, C: t.float().reshape(B, H, W, C).permute(0, 3, 1, 2)   # noqa: E731  (a channels-last NCHW view)
            o32, o3 = conv_run(x3, nchw(x, Ci), w.float().reshape(Co, Ci, 1, 1), nchw(dy, Co), Ci)
            got = {"y": o3["y"].permute(0, 2, 3, 1).reshape(M, Co), "dx": o3["dx"].permute(0, 2, 3, 1).reshape(M, Ci), "dw": o3["dw"].reshape(Co, Ci)}
            for n in ("y", "dx", "dw"):
                bad = got[n] != ref[n].float()
                print(f"[x3] conv_nobias {Ci}->{Co} M={M} {pattern} {n}: {int(bad.sum())} of {bad.numel()} elements differ from float64")
                if bool(bad.any()):
                    r, c = (int(v) for v in torch.nonzero(bad)[0])
                    fail.append(f"{Ci}->{Co} M={M} {pattern} {n}: {int(bad.sum())} of {bad.numel()} elements differ, the first at [{r}][{c}]: "
                                f"{float(got[n][r, c]):.1f} for {float(ref[n][r, c]):.1f}; rows {sorted(set(torch.nonzero(bad)[:, 0].tolist()))[:8]}.., "
                                f"columns {sorted(set(torch.nonzero(bad)[:, 1].tolist()))[:8]}..")
    assert not fail, f"{len(fail)} result(s) not bit-equal to float64:\n" + "\n".join(fail)


# ---- 2. NAFBlock (nafblock.hip), C >= 256: no LayerNorm in an epilogue, no fused narrow-level chain ---------------------------------------
# forward   conv1 A_PLAIN/E_BIAS (M, 2C) | conv3 A_SCALE/E_RESID (M, C): split3 with kscale, one problem and one split image per image |
#           conv4 A_PLAIN/E_BIASGATE (M, 2C) | conv5 A_PLAIN/E_RESID (M, C):  N = C or 2C, K = C: all four in the mode
# backward  B1 A_PLAIN/E_SGBWD (M, C) | B3 E_PLAIN (M, C; K = 2C) | B6 E_DOTCOL where an image is whole 128-pixel tiles, else E_PLAIN (M, C) |
#           B11 E_PLAIN (M, C; K = 2C): all four in the mode
# weight gradients, all with column sums: conv5 (C, C) | conv4 (2C, C) | conv1 (2C, C): plain operands, in the mode;
#           conv3 (C, C): plain operands and in the mode iff the splits can be image-aligned (P % 32 == 0, gemm_tn_plan_images; P = 128: two
#           splits of 128 rows), otherwise the scaled-operand loader (A_SCALE), which the mode does not take: fp32 128 x 128
#   (2, 256, 16, 8)  P = 128, M = 256: the E_DOTCOL form, one 256-row tile holding both images
#   (3, 256, 5, 7)   P = 35, nimg = 3, M = 105: every tile ragged, B6 E_PLAIN, conv3's weight gradient fp32
#   (1, 512, 8, 9)   P = M = 72, K = 512 / 1024: TN tiles two wide along K, the column sums of X shared between the blocks of a tile row
NAF = [((2, 256, 16, 8), {"x3": 8}, {"x3": 4}),
       ((3, 256, 5, 7), {"x3": 8}, {"x3": 3, "128x128": 1}),
       ((1, 512, 8, 9), {"x3": 8}, {"x3": 3, "128x128": 1})]
NAF_IN_MODE = ["conv1.weight", "conv1.bias", "conv3.weight", "conv3.bias", "beta", "conv4.weight", "conv4.bias", "conv5.weight", "conv5.bias", "gamma"]


def nafblock_case(dev, x3, shape, nt, tn, pass_, seed=0):
    from dcpt_amd import functional as DF

    c = shape[1]
    P0 = {k: keyed_tensor(f"x3ops{c}." + k, tuple(v.shape), seed).to(dev) for k, v in TPA.block_params(c, "").items()}
    x, go, P = block_inputs(dev, shape, P0, pass_, seed)
    Pr, xr = {k: f64(v) for k, v in P.items()}, f64(x)
    yr = O.nafblock(xr, Pr, "")
    yr.backward(go.double())

    def op():
        Pg, xg = {k: v.clone().requires_grad_(True) for k, v in P.items()}, x.clone().requires_grad_(True)
        y = DF.nafblock(xg, {fk: Pg[rk] for fk, rk in TPA.FUSED.items()})
        y.backward(go)
        return {"y": y.detach(), "dx": xg.grad, **{"grad " + k: v.grad for k, v in Pg.items()}}

    o32, o3 = both_modes(x3, op, nt, tn)
    label = f"nafblock {shape} {pass_}"
    rep, rat = Report(TPA, label), Ratio(label, "nafblock", pass_)
    ref = {"y": yr, "dx": xr.grad, **{"grad " + k: v.grad for k, v in Pr.items()}}
    for n, tol in [("y", 2e-5), ("dx", 5e-5)] + [("grad " + k, 1e-4) for k in P]:
        rep.cmp(n, o3[n], ref[n], tol)
    conv3_in_mode = shape[2] * shape[3] % 32 == 0
    for n in ["y", "dx"] + ["grad " + k for k in NAF_IN_MODE if conv3_in_mode or k not in ("conv3.weight", "conv3.bias", "beta")]:
        rat.cmp(n, o32[n], o3[n], ref[n])
    return rep, rat


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("shape,nt,tn", NAF)
def test_nafblock(dev, x3, shape, nt, tn, pass_):
    for r in nafblock_case(dev, x3, shape, nt, tn, pass_):
        r.done()


# ---- 3. the TLSC inference form (dcpt_nafblock_local_fwd): SCA's global mean is a k1 x k2 box mean, the scale a per-pixel map out of a GEMM ---
#   conv1 A_PLAIN/E_BIAS (M, 2C) | smap = Wsca boxmean(t2) + bsca, times t2: A_PLAIN/E_MUL (M, C) | conv3 A_PLAIN/E_RESID (M, C)
#   | conv4 A_PLAIN/E_BIASGATE (M, 2C) | conv5 A_PLAIN/E_RESID (M, C);  no backward.  C = 256: all five in the mode
def local_case(dev, x3, pass_, seed=0):
    from dcpt_amd import functional as DF

    shape, k1, k2 = (2, 256, 12, 10), 5, 4
    c = shape[1]
    P0 = {k: keyed_tensor(f"x3ops{c}." + k, tuple(v.shape), seed).to(dev) for k, v in TPA.block_params(c, "").items()}
    x, _, P = block_inputs(dev, shape, P0, pass_, seed)
    with torch.no_grad():   # nafnet_oracle.nafblock in float64 with the pooled mean replaced by the box-mean map (tests/test_gpu_gemm_tiles.py)
        g = {k: v.double() for k, v in P.items()}
        xd = x.double()
        t = F.conv2d(O.layernorm2d(xd, g["norm1.weight"], g["norm1.bias"]), g["conv1.weight"], g["conv1.bias"])
        t = O.simple_gate(F.conv2d(t, g["conv2.weight"], g["conv2.bias"], padding=1, groups=2 * c))
        t = t * F.conv2d(TTL._box_mean_f64(t, k1, k2), g["sca.1.weight"], g["sca.1.bias"])
        y1 = xd + F.conv2d(t, g["conv3.weight"], g["conv3.bias"]) * g["beta"]
        t = O.simple_gate(F.conv2d(O.layernorm2d(y1, g["norm2.weight"], g["norm2.bias"]), g["conv4.weight"], g["conv4.bias"]))
        yr = y1 + F.conv2d(t, g["conv5.weight"], g["conv5.bias"]) * g["gamma"]

        def op():
            return {"y": DF.nafblock_local(x, {fk: P[rk] for fk, rk in TPA.FUSED.items()}, k1, k2)}

        o32, o3 = both_modes(x3, op, {"x3": 5}, {})
    label = f"nafblock_local {shape} k={k1, k2} {pass_}"
    rep, rat = Report(TPA, label), Ratio(label, "local", pass_)
    rep.cmp("y", o3["y"], yr, 2e-5)
    rat.cmp("y", o32["y"], o3["y"], yr)
    return rep, rat


@pytest.mark.parametrize("pass_", PASSES)
def test_nafblock_local(dev, x3, pass_):
    for r in local_case(dev, x3, pass_):
        r.done()


# ---- 4. Restormer / PromptIR TransformerBlock (restormer.hip), the default ("balanced") save mode, (2, dim, 5, 7): P = 35, M = 70 -----------
# c = dim, ch = c / heads = 256, hp = int(2.66 c) rounded up to 4; no weight gradient carries column sums (no biases)
# MDTA  fwd qkv A_PLAIN/E_PLAIN (M, 3c) | attn @ v, BATCHED per (image, head) (P, ch; K = ch), per-problem weights = the attention matrices
#           | proj A_PLAIN/E_RESID (M, c);  Gram matrices: batched TN (ch, ch)
#       bwd attn @ v again (not kept) | d(att) (M, c) | dv batched (P, ch) | dq, dk A_PLAIN/E_ADDSCALED batched (P, ch), cscale strided per
#           (image, head) | d(LN x) (M, c; K = 3c):  all nine NT launches have N % 256 == 0 and K % 64 == 0: in the mode
#           dW proj (c, c) | dW qkv (3c, c): in the mode;  Gram and dattn: batched, which the TN kernel of the mode does not take: fp32 128 x 128
# GDFN  fwd project_in (M, 2hp) | project_out A_PLAIN/E_RESID (M, c; K = hp);  bwd dt (M, hp) | d(LN x) (M, c; K = 2hp);  dW out (c, hp) | dW in (2hp, c)
#       hp = 1364 (c = 512) / 680 (c = 256): N = hp, 2hp are no multiples of 256 and K = hp, 2hp none of 64: all four NT launches stay fp32
#       (128 x 64 at these grids), and so do both weight gradients:
#       c = 512: dW in (2728, 512) pads least on 96 x 128, dW out (512, 1364) on 128 x 128
#       c = 256: dW in (1360, 256) and dW out (256, 680: 768 padded either way) 128 x 128
#   dim 512, 2 heads: nb1 * nb2 = 4 problems, four split images in the scratch;  dim 256, 1 head: nb1 * nb2 = 2, N = 768 / 256
TB_LAUNCHES = {(512, 2): ({"x3": 9, "128x64": 4}, {"x3": 2, "128x128": 3, "96x128": 1}),
               (256, 1): ({"x3": 9, "128x64": 4}, {"x3": 2, "128x128": 4})}
TB_IN_MODE = ["attn.qkv.weight", "attn.project_out.weight"]
# the block of restormer_arch (ReLU-normalised attention, LayerNorm eps 1e-6) in both LayerNorm types, and PromptIR's (softmax attention,
# eps 1e-5; ch = 256 is the widest head the softmax kernels take), each with its own module's tolerances (y, dx, parameter gradients)
TB_KINDS = {"restormer BiasFree": ("BiasFree", False, 2e-4, 3e-4), "restormer WithBias": ("WithBias", False, 2e-4, 3e-4),
            "promptir WithBias": ("WithBias", True, 3e-4, 5e-4)}


def relu_attention_margin(x, P):
    """the smallest |pre-activation| of MDTA's ReLU over the largest, in float64 (restormer_oracle.attention up to its ReLU)"""
    with torch.no_grad():
        Pd = {k: v.double() for k, v in P.items()}
        t = R.layernorm(x.double(), Pd, "norm1.")
        b, c, h, w = t.shape
        heads = Pd["attn.temperature"].shape[0]
        qkv = F.conv2d(F.conv2d(t, Pd["attn.qkv.weight"]), Pd["attn.qkv_dwconv.weight"], padding=1, groups=3 * c)
        q, k, _ = qkv.chunk(3, dim=1)
        q, k = (F.normalize(u.reshape(b, heads, c // heads, h * w), dim=-1) for u in (q, k))
        z = (q @ k.transpose(-2, -1)) * Pd["attn.temperature"]
        return float(z.abs().min() / z.abs().max())


def transformer_inputs(dev, dim, P0, pass_, seed, softmax, rel=1e-6, rounds=40):
    """ReLU's derivative is a step (settle_relu of tests/test_gpu_gemm_tiles.py): with 131 072 - 262 144 entries in the attention maps,
    about one draw in two to four has an entry within fp32 rounding (~1e-7 of the largest) of zero, which the fp32 kernels and float64 then
    put on different sides -- dx and the qkv gradients move by 1e-3 and no fp32 result can be held to them (seen in both modes).  The
    whole map feeds every entry, so the inputs are drawn again, as a whole, until no pre-activation lies within ``rel`` of zero."""
    for draw in range(rounds):
        x, go, P = block_inputs(dev, (2, dim, 5, 7), P0, pass_, seed + 100 * draw, vspan=8)   # (8: the module docstring)
        if softmax or relu_attention_margin(x, P) >= rel:
            return x, go, P
    raise AssertionError(f"a pre-activation of the attention's ReLU within {rel:.0e} of zero in each of {rounds} draws")


def transformer_case(dev, x3, kind, dim, heads, pass_, seed=0):
    lnt, softmax, tol_dx, tol_g = TB_KINDS[kind]
    if softmax:
        from basicsr.archs.promptir_arch import TransformerBlock
    else:
        from basicsr.archs.restormer_arch import TransformerBlock
    mod, oracle = (TPR, PO) if softmax else (TRS, R)
    blk = TransformerBlock(dim, heads, 2.66, False, lnt)
    P0 = {k: keyed_tensor(f"x3ops{dim}." + k, tuple(v.shape), seed).to(dev) for k, v in blk.state_dict().items()}
    x, go, P = transformer_inputs(dev, dim, P0, pass_, seed, softmax)
    blk.load_state_dict(P, strict=True)
    blk = blk.to(dev)
    Pr, xr = {k: f64(v) for k, v in P.items()}, f64(x)
    yr = oracle.transformer_block(xr, Pr, "")
    yr.backward(go.double())

    def op():
        xg = x.clone().requires_grad_(True)
        for p in blk.parameters():
            p.grad = None
        y = blk(xg)
        y.backward(go)
        return {"y": y.detach(), "dx": xg.grad, **{"grad " + k: p.grad.clone() for k, p in blk.named_parameters()}}

    o32, o3 = both_modes(x3, op, *TB_LAUNCHES[(dim, heads)])
    label = f"{kind} dim {dim} heads {heads} {pass_}"
    rep, rat = Report(mod, label), Ratio(label, "transformer", pass_)
    ref = {"y": yr, "dx": xr.grad, **{"grad " + k: v.grad for k, v in Pr.items()}}
    for n, tol in [("y", 5e-5), ("dx", tol_dx)] + [("grad " + k, tol_g) for k, _ in blk.named_parameters()]:
        rep.cmp(n, o3[n], ref[n], tol)
    for n in ["y", "dx"] + ["grad " + k for k in TB_IN_MODE]:
        rat.cmp(n, o32[n], o3[n], ref[n])
    return rep, rat


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("dim,heads", [(512, 2), (256, 1)])
@pytest.mark.parametrize("kind", list(TB_KINDS))
def test_transformer_block(dev, x3, kind, dim, heads, pass_):
    for r in transformer_case(dev, x3, kind, dim, heads, pass_):
        r.done()
