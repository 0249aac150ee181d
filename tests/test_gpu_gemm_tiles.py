"""Which fp32 GEMM tile produced the result?  launch_gemm_nt picks one of three kernels per launch (128 x 64, 128 x 96, 128 x 128;
nt_pick_bn, dcpt_amd/csrc/gemm_nt.hip) from the size of the grid, launch_gemm_tn one of six (tn_tile_shape, gemm_tn.hip); every
(loader, epilogue, width) is an instantiation of its own and the epilogue's thread -> row map depends on the width.  The other
operator-level tests run at a few hundred to ~10 000 rows, where every NT launch takes the 128 x 64 kernel.  Here each public op runs at
the SMALLEST shape that puts its GEMMs on the wider kernel, with a ragged last row tile (M % 128 != 0) and, where the op's widths allow
it, a partial last column tile: under the red zone (tests/redzone.py), with the launch trace asserting the tag AND the count of every
fp32 GEMM family (tests/kernel_trace.py; the counts are hard-coded beside the list of the op's GEMMs, so a threshold edit fails the test
instead of re-routing it), and compared with the float64 restatement its own test module holds, computed on the device, at that module's
fp32 tolerances.

In the comments rt = cdiv(M, 128) is the number of row tiles; "96" / "128" / "64" the width nt_pick_bn gives the launch:
  96   iff  N > 64, cdiv(N, 96) * 96 < cdiv(N, 128) * 128  and  rt * cdiv(N, 96) * nbatch > 256      (never E_BIASGATE / E_LNBWD / E_RESIDLN)
  128  iff  N > 64 and rt * cdiv(N, 128) * nbatch >= 2100   (E_BIASGATE: rt * cdiv(N / 2, 64));  E_LNBWD / E_RESIDLN: iff N > 64
  64   otherwise.
A weight gradient (TN) with column sums or a transformed operand takes 128 / 64-wide tiles by its N and K alone; a plain one without
column sums (Restormer, PromptIR, the DCPT head) the 96-wide ones where they pad less.

Tiles that can never widen: conv3x3_act, up2_conv3x3_act, conv3x3_ps_out and conv3conv_res have N <= 64 at the networks' widths
(nt_pick_bn returns 64 for N <= 64 whatever the grid), so tests/test_gpu_swinir_sr.py and the sweep of tests/test_gpu_bounds.py already
run the only kernel they can take; they are not tested again here."""
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_tensor
from kernel_trace import kernel_trace
from oracle import dc_oracle as D
from oracle import nafnet_oracle as O
from oracle import promptir_oracle as PO
from oracle import restormer_oracle as R
from redzone import redzone
from tests import test_gpu_dchead as TDC
from tests import test_gpu_parity as TPA
from tests import test_gpu_promptir as TPR
from tests import test_gpu_rcan as TRC
from tests import test_gpu_restormer as TRS
from tests import test_gpu_swinir as TSW
from tests import test_gpu_tlsc_bf16 as TTL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def rand(dev, shape, seed):
    """uniform [-1, 1) NHWC map drawn on the device (the keyed generator is a host loop: seconds at these sizes)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(shape, generator=g, device=dev) * 2 - 1).contiguous(memory_format=torch.channels_last)


def f64(t):
    return t.detach().double().requires_grad_(True)


def settle_relu(x, preact, seed, rel=1e-5, rounds=12):
    """ReLU's derivative is a step: where a pre-activation lies within fp32 rounding of zero, the fp32 kernel and the float64 restatement
    may take different sides, and ONE such element moves dx by percents of its maximum and a weight gradient by one whole term of its
    sum (seen here: 4e-2 / 1e-3 with ~20 of 3.4e7 elements that close, while the same GEMMs without a ReLU agree to 1e-6).  Such an input has no
    gradient an fp32 result can be held to, so the map is drawn until none is left: every pixel at which |float64 pre-activation| <
    ``rel`` * max -- ten times the forward's fp32 error and more -- is drawn again (a 3 x 3 conv moves its neighbours too, hence the loop).
    ``preact`` maps the float64 input to the tensor the ReLU is applied to."""
    g = torch.Generator(device=x.device).manual_seed(seed)
    for _ in range(rounds):
        with torch.no_grad():
            z = preact(x.double())
            near = (z.abs() < rel * z.abs().max()).any(1, keepdim=True)
            if not bool(near.any()):
                return x
            fresh = torch.rand(x.shape, generator=g, device=x.device) * 2 - 1
            x = torch.where(near, fresh, x).contiguous(memory_format=torch.channels_last)
    raise AssertionError(f"{int(near.sum())} pixels still hold a pre-activation within {rel:.0e} of zero after {rounds} draws")


def assert_gemms(tr, nt, tn):
    """the fp32 GEMM families that ran, and how often: exactly these"""
    got_nt = {k[len("nt_f32."):]: v for k, v in tr.families("nt_f32.").items()}
    got_tn = {k[len("tn_f32."):]: v for k, v in tr.families("tn_f32.").items()}
    print(f"[tiles] launched nt {got_nt} tn {got_tn}")
    assert got_nt == nt, f"fp32 NT launches {got_nt}, expected {nt}"
    assert got_tn == tn, f"fp32 TN launches {got_tn}, expected {tn}"


def _err(a, b, scale):
    """'max error / scale' over the finite elements of a, and how many are not (the red zone starts every output as NaNs)"""
    if not a.numel():
        return "-"
    d = (a.double() - b).abs()
    bad = int((~torch.isfinite(d)).sum())
    return f"{float(torch.nan_to_num(d, nan=0.0, posinf=0.0).max() / scale):.3e}" + (f" and {bad} non-finite" if bad else "")


class Report:
    """Every comparison of a case through ``mod.check`` (the test module's own scale-relative max error), each figure printed before
    anything is asserted; a failure also says how much of the error lies in the rows of the last row tile (pixels >= (M // 128) * 128
    of an activation) and in the columns of the last column tile of width ``bn``, and the case fails at the end with every miss."""

    def __init__(self, mod, label):
        self.mod, self.label, self.fail = mod, label, []

    def cmp(self, name, a, b, tol, bn=128):
        a, b = a.detach(), b.detach()
        scale = max(1e-12, float(b.abs().max()))
        print(f"[tiles] {self.label} {name}: err {_err(a, b, scale)} (tol {tol:.1e})")
        try:
            self.mod.check(name, a, b, tol)
        except AssertionError as ex:
            self.fail.append(str(ex).split("\n")[0] + self.tail(a, b, scale, bn))

    @staticmethod
    def tail(a, b, scale, bn):
        if a.dim() == 4 and a.shape[2] * a.shape[3] > 9:   # an activation (no 3 x 3 weight): rows are pixels, columns channels
            C = a.shape[1]
            ra, rb = a.permute(0, 2, 3, 1).reshape(-1, C), b.permute(0, 2, 3, 1).reshape(-1, C)
        else:                                              # a parameter gradient [N][K...]: one GEMM column per output channel
            ra, rb = a.reshape(a.shape[0], -1).t(), b.reshape(b.shape[0], -1).t()
        M, N = ra.shape
        r0, c0 = (M // 128) * 128, ((N - 1) // bn) * bn
        return (f"  [rows >= {r0} of {M}: {_err(ra[r0:], rb[r0:], scale)}, rows below: {_err(ra[:r0], rb[:r0], scale)}; "
                f"columns >= {c0} of {N} ({bn}-wide tiles): {_err(ra[:, c0:], rb[:, c0:], scale)}, "
                f"columns below: {_err(ra[:, :c0], rb[:, :c0], scale)}]")

    def done(self):
        assert not self.fail, f"{self.label}: {len(self.fail)} comparison(s) missed:\n" + "\n".join(self.fail)


# ---- NAFBlock (nafblock.hip) ------------------------------------------------------------------------------------------------------------
# forward   conv1 A_PLAIN/E_BIAS (M, 2C) | conv3 A_SCALE/E_RESIDLN (C <= 128) or A_SCALE/E_RESID (M, C) | conv4 A_PLAIN/E_BIASGATE (M, 2C)
#           | conv5 A_PLAIN/E_RESID (M, C)
# backward  B1 A_PLAIN/E_SGBWD (M, C) | B3 A_PLAIN/E_LNBWD (C <= 128) or E_PLAIN (M, C) | B6 A_PLAIN/E_DOTCOL (images of whole 128-pixel
#           tiles) or E_PLAIN (M, C) | B11 A_PLAIN/E_LNBWD or E_PLAIN (M, C);  weight gradients (all with column sums): conv5 (C, C),
#           conv4 (2C, C), conv3 (C, C), conv1 (2C, C)
# (1, 128, 403, 667): M = 268 801 = 2100 * 128 + 1, rt = 2101 >= 2100: every launch is 128-wide, N = 128 one and N = 256 two column tiles
# (1, 512, 67, 1003): M = 67 201 = 525 * 128 + 1, rt = 526, N = 512 / 1024: 2104 / 4208 tiles, K = 512 / 1024
# (3, 128, 128, 701): P = 701 * 128, M = 2103 * 128: no ragged tile, but the only way to E_DOTCOL (P % 128 == 0) on the 128-wide tile
NAF = [(1, 128, 403, 667), (1, 512, 67, 1003), (3, 128, 128, 701)]


@pytest.mark.parametrize("B,c,H,W", NAF)
def test_nafblock_fp32_wide(dev, B, c, H, W):
    from dcpt_amd import functional as DF

    P = {k: v.to(dev) for k, v in TPA.block_params(c, f"tw{c}.").items()}
    x, go = rand(dev, (B, c, H, W), 1), rand(dev, (B, c, H, W), 2)
    Pr = {k: f64(v) for k, v in P.items()}
    xr = f64(x)
    yr = O.nafblock(xr, Pr, "")
    yr.backward(go.double())
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xg = x.clone().requires_grad_(True)
    with redzone() as rz, kernel_trace() as tr:
        y = DF.nafblock(xg, {fk: Pg[rk] for fk, rk in TPA.FUSED.items()})
        y.backward(go)
    assert rz.count > 0
    assert_gemms(tr, {"128x128": 8}, {"128x128": 4})
    rep = Report(TPA, f"nafblock {B, c, H, W}")
    rep.cmp("y", y, yr, 2e-5)
    rep.cmp("dx", xg.grad, xr.grad, 5e-5)
    for k in P:
        rep.cmp("grad " + k, Pg[k].grad, Pr[k].grad, 1e-4)
    # the no_grad path: the same four forward GEMMs (only the fused narrowest level, C = 64, has a form of its own without a backward)
    with torch.no_grad(), redzone() as rz, kernel_trace() as tr:
        yi = DF.nafblock(x, {fk: Pg[rk] for fk, rk in TPA.FUSED.items()})
    assert rz.count > 0
    assert_gemms(tr, {"128x128": 4}, {})
    rep.cmp("y (no_grad)", yi, yr, 2e-5)
    rep.done()


# TLSC inference form (dcpt_nafblock_local_fwd): SCA's global mean is a k1 x k2 box mean, the scale a per-pixel map out of a GEMM
#   conv1 A_PLAIN/E_BIAS (M, 2C) | smap = Wsca boxmean(t2) + bsca, times t2: A_PLAIN/E_MUL (M, C) | conv3 A_PLAIN/E_RESID (M, C)
#   | conv4 A_PLAIN/E_BIASGATE (M, 2C) | conv5 A_PLAIN/E_RESID (M, C);  no backward
def test_nafblock_local_fp32_wide(dev):
    from dcpt_amd import functional as DF

    B, c, H, W = NAF[0]
    k1, k2 = 3, 4
    P = {k: v.to(dev) for k, v in TPA.block_params(c, f"tw{c}.").items()}
    x = rand(dev, (B, c, H, W), 1)
    with torch.no_grad():   # nafnet_oracle.nafblock in float64 with the pooled mean replaced by the box-mean map (arch_util.py:378-396)
        g = {k: v.double() for k, v in P.items()}
        xd = x.double()
        t = F.conv2d(O.layernorm2d(xd, g["norm1.weight"], g["norm1.bias"]), g["conv1.weight"], g["conv1.bias"])
        t = O.simple_gate(F.conv2d(t, g["conv2.weight"], g["conv2.bias"], padding=1, groups=2 * c))
        t = t * F.conv2d(TTL._box_mean_f64(t, k1, k2), g["sca.1.weight"], g["sca.1.bias"])
        y1 = xd + F.conv2d(t, g["conv3.weight"], g["conv3.bias"]) * g["beta"]
        t = O.simple_gate(F.conv2d(O.layernorm2d(y1, g["norm2.weight"], g["norm2.bias"]), g["conv4.weight"], g["conv4.bias"]))
        yr = y1 + F.conv2d(t, g["conv5.weight"], g["conv5.bias"]) * g["gamma"]
        del t, y1, xd
        with redzone() as rz, kernel_trace() as tr:
            y = DF.nafblock_local(x, {fk: P[rk] for fk, rk in TPA.FUSED.items()}, k1, k2)
    assert rz.count > 0
    tr.assert_ran("tlsc.box_mean_f32")
    assert_gemms(tr, {"128x128": 5}, {})
    rep = Report(TPA, f"nafblock_local {B, c, H, W} k={k1, k2}")
    rep.cmp("y", y, yr, 2e-5)
    rep.done()


# ---- down / up sampling (capi.hip) ------------------------------------------------------------------------------------------------------
# coarse grid 213 x 631: Mc = 134 403 = 1050 * 128 + 3, rt = 1051; 128-wide needs two column tiles of 128 (2102 >= 2100)
# down2x2, C = 128   fwd A_GATHER/E_BIAS (Mc, 256) 128 | bwd A_PLAIN/E_SCATTER (Mc, 512) 128, E_SCATTER_ADD in down2x2_skip
#                    | dW: X plain, Y gathered (256, 512), column sums
# up_ps, C = 128     fwd A_PLAIN/E_SCATTER_ADD (Mc, 256) 128 | bwd A_GATHER/E_PLAIN (Mc, 128): ONE column tile, 1051 < 2100: 64
#                    | dW: X gathered (256, 128)
# up_ps, C = 256     fwd (Mc, 512) 128 | bwd A_GATHER/E_PLAIN (Mc, 256) 128 | dW (512, 256)
GH, GW = 213, 631


def test_down2x2_wide(dev):
    from dcpt_amd import functional as DF

    C, H, W = 128, 2 * GH, 2 * GW
    x, go, gs = rand(dev, (1, C, H, W), 3), rand(dev, (1, 2 * C, GH, GW), 4), rand(dev, (1, C, H, W), 5)
    w, b = keyed_tensor("tw.downs.weight", (2 * C, C, 2, 2)).to(dev), keyed_tensor("tw.downs.bias", (2 * C,)).to(dev)
    xr, wr, br = f64(x), f64(w), f64(b)
    yr = F.conv2d(xr, wr, br, stride=2)
    yr.backward(go.double())
    rep = Report(TPA, "down2x2")
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, b))
    with redzone() as rz, kernel_trace() as tr:
        y = DF.down2x2(xg, wg, bg)
        y.backward(go)
    assert rz.count > 0
    assert_gemms(tr, {"128x128": 2}, {"128x128": 1})
    rep.cmp("down y", y, yr, 1e-5)
    rep.cmp("down dx", xg.grad, xr.grad, 1e-5)
    rep.cmp("down dw", wg.grad, wr.grad, 1e-5)
    rep.cmp("down db", bg.grad, br.grad, 1e-5)
    # the encoder output's two consumers as one node: the skip's gradient joins in the scatter epilogue (E_SCATTER_ADD)
    x2, w2, b2 = (t.clone().requires_grad_(True) for t in (x, w, b))
    with redzone() as rz, kernel_trace() as tr:
        y2, skip = DF.down2x2_skip(x2, w2, b2)
        torch.autograd.backward([y2, skip], [go, gs])
    assert rz.count > 0
    assert_gemms(tr, {"128x128": 2}, {"128x128": 1})
    assert torch.equal(y2, y) and torch.equal(w2.grad, wg.grad) and torch.equal(b2.grad, bg.grad)
    rep.cmp("down_skip dx", x2.grad, xr.grad + gs.double(), 1e-5)
    rep.done()


@pytest.mark.parametrize("C,nt", [(128, {"128x128": 1, "128x64": 1}), (256, {"128x128": 2})])
def test_up_ps_wide(dev, C, nt):
    from dcpt_amd import functional as DF

    x, skip, go = rand(dev, (1, C, GH, GW), 6), rand(dev, (1, C // 2, 2 * GH, 2 * GW), 7), rand(dev, (1, C // 2, 2 * GH, 2 * GW), 8)
    w = keyed_tensor("tw.ups.weight", (2 * C, C, 1, 1)).to(dev)
    xr, wr, sr = f64(x), f64(w), f64(skip)
    yr = O.pixel_shuffle2(F.conv2d(xr, wr)) + sr
    yr.backward(go.double())
    xg, wg, sg = (t.clone().requires_grad_(True) for t in (x, w, skip))
    with redzone() as rz, kernel_trace() as tr:
        y = DF.up_ps(xg, wg, sg)
        y.backward(go)
    assert rz.count > 0
    assert_gemms(tr, nt, {"128x128": 1})
    rep = Report(TPA, f"up_ps C={C}")
    rep.cmp("up y", y, yr, 1e-5)
    rep.cmp("up dx", xg.grad, xr.grad, 1e-5)
    rep.cmp("up dw", wg.grad, wr.grad, 1e-5)
    rep.cmp("up dskip", sg.grad, sr.grad, 1e-6)
    rep.done()


# ---- SwinIR block and RSTB conv, C = 180, 6 heads, window 8 (swin.hip) -----------------------------------------------------------------
# attention  fwd qkv A_LN/E_BIAS (M, 540) | proj A_PLAIN/E_RESID (M, 180);  bwd d(att) A_PLAIN/E_PLAIN (M, 180) | d(LN1 x) A_PLAIN/E_PLAIN
#            (M, 180; K = 540);  dW proj (180, 180), qkv (540, 180; LayerNorm in the loader)
# MLP        fwd fc1 A_LN/E_BIAS (M, 360) | fc2 A_PLAIN/E_RESID (M, 180);  bwd d(gelu) A_PLAIN/E_PLAIN (M, 360) | d(LN2 x) A_PLAIN/E_PLAIN
#            (M, 180; K = 360);  dW fc2 (180, 360), fc1 (360, 180; LayerNorm in the loader)
# conv       fwd A_CONV3/E_RESID (M, 180; K = 1620);  bwd A_CONV3/E_PLAIN (M, 180);  dW (180, 1620; implicit conv in the loader)
# every weight gradient carries column sums (the bias gradients): 128 x 128 tiles, never the 96-wide ones
# N = 540 pads to 576 (< 640): 96-wide above 256 tiles, last column tile 60 wide;  N = 180 pads to 192 (< 256): last column tile 84 wide
# N = 360 pads to 384 either way: never 96; 128-wide from rt * 3 >= 2100, last column tile 104 wide
#   (136, 136)  M = 18 496 = 144 * 128 + 64, rt = 145:  N = 540: 870 tiles, N = 180: 290 tiles: 96;  N = 360: 435 < 2100: 64
#   (296, 312)  M = 92 352 = 721 * 128 + 64, rt = 722:  N = 360: 2166 >= 2100: 128
#   (128, 128)  M = 16 384, rt = 128 (the control): N = 180: exactly 256 tiles, NOT above 256: 64; the forward qkv (N = 540, 768 tiles) is the
#               one launch of the block that stays 96-wide (its dgrad has N = 180)
SWIN = [(136, 136, {"128x96": 6, "128x64": 2}, {"128x96": 2}),
        (296, 312, {"128x96": 6, "128x128": 2}, {"128x96": 2}),
        (128, 128, {"128x96": 1, "128x64": 7}, {"128x64": 2})]


@pytest.mark.parametrize("H,W,nt_block,nt_conv", SWIN)
def test_swinir_block_and_conv_wide(dev, H, W, nt_block, nt_conv):
    from basicsr.archs.swinir_arch import SwinTransformerBlock
    from dcpt_amd import functional as DF

    C, heads, ws = 180, 6, 8
    x, go = rand(dev, (1, C, H, W), 9), rand(dev, (1, C, H, W), 10)
    rep = Report(TSW, f"swinir {H}x{W}")
    for shift in (0, ws // 2):
        blk = SwinTransformerBlock(C, (128, 128), heads, ws, shift, 2.0)
        fill_module_(blk, seed=C + shift)
        blk = blk.to(dev)
        P = {k: f64(v) for k, v in blk.state_dict().items()}
        xr, xg = f64(x), x.clone().requires_grad_(True)
        yr = TSW.ref_block(xr, P, "", heads, ws, shift)
        yr.backward(go.double())
        with redzone() as rz, kernel_trace() as tr:
            y = blk(xg)
            y.backward(go)
        assert rz.count > 0
        tr.assert_ran("swin_wattn_fwd", "swin_wattn_bwd")
        assert_gemms(tr, nt_block, {"128x128": 4})
        rep.cmp(f"y shift={shift}", y, yr, 5e-5, bn=96)
        rep.cmp(f"dx shift={shift}", xg.grad, xr.grad, 2e-4, bn=96)
        for k, p in blk.named_parameters():
            rep.cmp(f"grad {k} shift={shift}", p.grad, P[k].grad, 3e-4)
        del P, xr, yr, y
    w, b = keyed_tensor("tw.conv.weight", (C, C, 3, 3)).to(dev), keyed_tensor("tw.conv.bias", (C,)).to(dev)
    res = rand(dev, (1, C, H, W), 11)
    ref = [f64(t) for t in (x, w, b, res)]
    yr = F.conv2d(ref[0], ref[1], ref[2], padding=1) + ref[3]
    yr.backward(go.double())
    gpu = [t.clone().requires_grad_(True) for t in (x, w, b, res)]
    with redzone() as rz, kernel_trace() as tr:
        y = DF.conv3x3_res(*gpu)
        y.backward(go)
    assert rz.count > 0
    tr.assert_ran("swin_conv3x3_res_fwd", "swin_conv3x3_res_bwd")
    assert_gemms(tr, nt_conv, {"128x128": 1})
    rep.cmp("conv y", y, yr, 5e-5, bn=96)
    for n, a, r in zip(["conv dx", "conv dw", "conv db", "conv dres"], gpu, ref):
        rep.cmp(n, a.grad, r.grad, 2e-4 if n in ("conv dx", "conv dres") else 3e-4, bn=96)
    rep.done()


# ---- Restormer / PromptIR block (restormer.hip), the default ("balanced") save mode, M = 182 * 181 = 32 942 = 257 * 128 + 46, rt = 258 ------
# c = dim, ch = c / heads, hp = hidden rounded up to 4; no weight gradient carries column sums (no biases), so the plain ones take 96-wide tiles
# MDTA  fwd qkv A_PLAIN/E_PLAIN (M, 3c) | attn @ v, batched per head (P, ch) | proj A_PLAIN/E_RESID (M, c);  Gram matrices TN (ch, ch) batched
#       bwd attn @ v again (not kept) | d(att) (M, c) | dv batched (P, ch) | dq, dk A_PLAIN/E_ADDSCALED batched (P, ch) twice | d(LN x) (M, c; K = 3c)
#           dW proj (c, c) | dattn batched (ch, ch) | dW qkv (3c, c)
# GDFN  fwd project_in A_PLAIN/E_PLAIN (M, 2hp) | project_out A_PLAIN/E_RESID (M, c; K = hp)
#       bwd dt (M, hp) | d(LN x) (M, c; K = 2hp);  dW out (c, hp) | dW in (2hp, c)
# dim 96, 1 head (ch = 96, hp = 256): N = 96 (258 tiles > 256) and 288 (774): 96;  N = 512 (rt * 4 = 1032), N = 256 (516): 64
#     NT 96: qkv, attn @ v (twice), proj, d(att), dv, dq, dk, d(LN x), project_out, d(LN x) of GDFN = 11;  64: project_in, dt = 2
#     TN (ch, ch) = (96, 96) twice, (96, 96), (288, 96), (512, 96): 128 x 96;  (96, 256): 96 x 128
# dim 48, 1 head (ch = 48, hp = 128): only qkv (N = 144 pads to 192 < 256, 516 tiles) is 96-wide; N = 48 / 128 / 256: 64
#     NT 96: 1;  64: attn @ v (twice), proj, d(att), dv, dq, dk, d(LN x), project_in, project_out, dt, d(LN x) = 12
#     TN (48, 48) three times: 64 x 64;  (144, 48), (256, 48): 128 x 64;  (48, 128): 64 x 128
# PromptIR dim 160, 4 heads (ch = 40, hp = 428): N = 480 (qkv), 160, 856 (pads to 864 < 896), 428 (480 < 512): 96;  the per-head N = 40: 64.
#     (PromptIR's N = 320 pads to 384 either way and never takes the 96-wide tile)
#     NT 96: qkv, proj, d(att), d(LN x), project_in, project_out, dt, d(LN x) = 8;  64: attn @ v (twice), dv, dq, dk = 5
#     TN (40, 40) twice: 64 x 64;  (160, 160), (480, 160), (856, 160): 128 x 96;  (160, 428): 96 x 128
RH, RW = 182, 181
RESTORMER = {96: ({"128x96": 11, "128x64": 2}, {"128x96": 5, "96x128": 1}),
             48: ({"128x96": 1, "128x64": 12}, {"64x64": 3, "128x64": 2, "64x128": 1})}


def _transformer_block(dev, mod, oracle, blk, dim, nt, tn, label, tol_dx, tol_g):
    sd = {k: keyed_tensor(f"tw{label}." + k, tuple(v.shape)) for k, v in blk.state_dict().items()}
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev)
    x, go = rand(dev, (1, dim, RH, RW), 12), rand(dev, (1, dim, RH, RW), 13)
    P = {k: f64(v.to(dev)) for k, v in sd.items()}
    xr, xg = f64(x), x.clone().requires_grad_(True)
    yr = oracle.transformer_block(xr, P, "")
    yr.backward(go.double())
    with redzone() as rz, kernel_trace() as tr:
        y = blk(xg)
        y.backward(go)
    assert rz.count > 0
    assert_gemms(tr, nt, tn)
    rep = Report(mod, label)
    rep.cmp("y", y, yr, 5e-5, bn=96)
    rep.cmp("dx", xg.grad, xr.grad, tol_dx, bn=96)
    for k, p in blk.named_parameters():
        rep.cmp("grad " + k, p.grad, P[k].grad, tol_g, bn=96)
    rep.done()


@pytest.mark.parametrize("dim", [96, 48])
@pytest.mark.parametrize("lnt", ["BiasFree", "WithBias"])
def test_restormer_block_wide(dev, lnt, dim):
    from basicsr.archs.restormer_arch import TransformerBlock

    nt, tn = RESTORMER[dim]
    _transformer_block(dev, TRS, R, TransformerBlock(dim, 1, 2.66, False, lnt), dim, nt, tn, f"restormer {lnt} {dim}", 2e-4, 3e-4)


def test_promptir_block_wide(dev):
    from basicsr.archs.promptir_arch import TransformerBlock

    _transformer_block(dev, TPR, PO, TransformerBlock(160, 4, 2.66, False, "WithBias"), 160, {"128x96": 8, "128x64": 5},
                       {"64x64": 2, "128x96": 3, "96x128": 1}, "promptir WithBias 160", 3e-4, 5e-4)


# ---- RCAN (rcan.hip) ----------------------------------------------------------------------------------------------------------------------
# RCAB(128, 16), (3, 128, 299, 300): P = 89 700 = 700 * 128 + 100 per image (the images straddle row tiles: E_BIASCOL's per-image column
#     sums), M = 269 100 = 2102 * 128 + 44, rt = 2103 >= 2100, N = 128: 128-wide
#     fwd A_CONV3/E_RELU (M, 128; K = 1152) | A_CONV3/E_BIASCOL (M, 128);  bwd A_CONV3/E_RELU (dh = [h > 0] conv2^T dt) | A_CONV3/E_RESID
#     (dx = dy + conv1^T dh);  dW conv2, conv1 (128, 1152; implicit conv in the loader, column sums)
def test_rcab_wide(dev):
    from basicsr.archs.rcan_arch import RCAB

    C, sq, B, H, W = 128, 16, 3, 299, 300
    blk = RCAB(C, sq, 0.5)
    fill_module_(blk, seed=C + H)
    blk = blk.to(dev)
    P = {k: f64(v) for k, v in blk.state_dict().items()}
    x, go = rand(dev, (B, C, H, W), 14), rand(dev, (B, C, H, W), 15)
    x = settle_relu(x, lambda t: F.conv2d(t, P["rcab.0.weight"], P["rcab.0.bias"], padding=1), 21)
    xr, xg = f64(x), x.clone().requires_grad_(True)
    yr = TRC.ref_rcab(xr, P, "", 0.5)
    yr.backward(go.double())
    with redzone() as rz, kernel_trace() as tr:
        y = blk(xg)
        y.backward(go)
    assert rz.count > 0
    tr.assert_ran("rcan_rcab_fwd", "rcan_rcab_bwd")
    assert_gemms(tr, {"128x128": 4}, {"128x128": 2})
    rep = Report(TRC, "rcab")
    rep.cmp("y", y, yr, 5e-5)
    rep.cmp("dx", xg.grad, xr.grad, 2e-4)
    for k, p in blk.named_parameters():
        rep.cmp("grad " + k, p.grad, P[k].grad, 3e-4)
    rep.done()


# Upsampler (conv3x3_ps), C = 64: fwd A_CONV3/E_PSHUF (M, r r 64; K = 576);  bwd A_CONV3/E_PLAIN (M, 64; K = 9 r r 64): N = 64, always 64-wide;
#     dW (r r 64, 576; implicit conv in the loader)
#   r = 3, (1, 64, 75, 74): M = 5550 = 43 * 128 + 46, rt = 44, N = 576 = 6 * 96 (< 640): 264 tiles > 256: 96
#   r = 2, (1, 64, 213, 631): rt = 1051, N = 256: 2102 >= 2100: 128
@pytest.mark.parametrize("r,H,W,wide", [(3, 75, 74, "128x96"), (2, GH, GW, "128x128")])
def test_rcan_upsampler_wide(dev, r, H, W, wide):
    from dcpt_amd import functional as DF

    C = 64
    x, go = rand(dev, (1, C, H, W), 16), rand(dev, (1, C, r * H, r * W), 17)
    w, b = keyed_tensor(f"tw.up{r}.weight", (r * r * C, C, 3, 3)).to(dev), keyed_tensor(f"tw.up{r}.bias", (r * r * C,)).to(dev)
    ref = [f64(t) for t in (x, w, b)]
    yr = F.pixel_shuffle(F.conv2d(ref[0], ref[1], ref[2], padding=1), r)
    yr.backward(go.double())
    gpu = [t.clone().requires_grad_(True) for t in (x, w, b)]
    with redzone() as rz, kernel_trace() as tr:
        y = DF.conv3x3_ps(gpu[0], gpu[1], gpu[2], r)
        y.backward(go)
    assert rz.count > 0
    tr.assert_ran("rcan_ps_fwd", "rcan_ps_bwd")
    assert_gemms(tr, {wide: 1, "128x64": 1}, {"128x128": 1})
    rep = Report(TRC, f"conv3x3_ps r={r}")
    rep.cmp("y", y, yr, 5e-5)
    rep.cmp("dx", gpu[0].grad, ref[0].grad, 2e-4)
    rep.cmp("dw", gpu[1].grad, ref[1].grad, 3e-4, bn=96 if r == 3 else 128)
    rep.cmp("db", gpu[2].grad, ref[2].grad, 3e-4, bn=96 if r == 3 else 128)
    rep.done()


# ---- DCPT head conv_ln (dchead.hip), 213 x 631: rt = 1051 ---------------------------------------------------------------------------------
# fwd ks 1 A_PLAIN/E_PLAIN, ks 3 A_CONV3/E_PLAIN (M, Cout);  bwd the same pair (M, Cin), behind the LayerNorm backward;  dW (Cout, ks ks Cin),
# no column sums
#   128 -> 256: fwd N = 256: 2102 tiles: 128;  bwd N = 128: ONE column tile, 1051 < 2100: 64
#   256 -> 256: the dgrad (N = 256) is 128-wide too
@pytest.mark.parametrize("Cin,Cout,ks,relu,res,nt", [(128, 256, 1, True, False, {"128x128": 1, "128x64": 1}),
                                                      (128, 256, 1, False, True, {"128x128": 1, "128x64": 1}),
                                                      (128, 256, 3, True, True, {"128x128": 1, "128x64": 1}),
                                                      (128, 256, 3, False, False, {"128x128": 1, "128x64": 1}),
                                                      (256, 256, 1, True, True, {"128x128": 2}),
                                                      (256, 256, 3, True, False, {"128x128": 2})])
def test_conv_ln_fp32_wide(dev, Cin, Cout, ks, relu, res, nt):
    from dcpt_amd import functional as DF

    x, go = rand(dev, (1, Cin, GH, GW), 18), rand(dev, (1, Cout, GH, GW), 19)
    ts = [x, keyed_tensor("tw.conv.weight", (Cout, Cin, ks, ks)).to(dev), keyed_tensor("tw.norm.weight", (Cout,)).to(dev),
          keyed_tensor("tw.norm.bias", (Cout,)).to(dev)] + ([rand(dev, (1, Cout, GH, GW), 20)] if res else [])
    ref = [f64(t) for t in ts]

    def preact(t):
        z = D.layernorm_cf(F.conv2d(t, ref[1], padding=ks // 2), ref[2], ref[3])
        return z + ref[4] if res else z

    if relu:
        ts[0] = settle_relu(x, preact, 22)
        ref[0] = f64(ts[0])
    yr = preact(ref[0])
    if relu:
        yr = F.relu(yr)
    yr.backward(go.double())
    gpu = [t.clone().requires_grad_(True) for t in ts]
    with redzone() as rz, kernel_trace() as tr:
        y = DF.conv_ln(gpu[0], gpu[1], gpu[2], gpu[3], gpu[4] if res else None, relu)
        y.backward(go)
    assert rz.count > 0
    assert_gemms(tr, nt, {"128x128": 1})
    rep = Report(TDC, f"conv_ln {Cin}->{Cout} ks{ks} relu={relu} res={res}")
    rep.cmp("y", y, yr, 2e-5)
    for n, a, b in zip(["dx", "dw", "dlnw", "dlnb", "dres"], gpu, ref):
        rep.cmp(n, a.grad, b.grad, 1e-4)
    rep.done()
