"""The fp32 SwinIR halves (dcpt_swin_attn_fwd / _bwd, dcpt_swin_mlp_fwd / _bwd; DF.swin_attn / DF.swin_mlp) and DF.img_affine stage by
stage against float64.

Each run calls one half directly on fp32 inputs, reads every tensor the forward keeps for the backward off ``y.grad_fn`` (mu, rstd, qkv,
att, lse; mu, rstd, h), runs the backward with a keyed dy and compares the stages, y, dx and every parameter gradient with the restatement
of tests/swin_restatement.py evaluated twice on the CPU from the same fp32 inputs: in float64 (the truth) and in float32 (the yardstick).
The runs, their inputs, the error measure and K live in tests/test_swin_restatement_cpu.py, which also ties the restatement to torch's own
ops and to the golden vectors of the real reference, asserts what this file states about its inputs, and asserts which run tells which
deliberate mistake from the right thing.

ERROR MEASURE (that of tests/test_gpu_restormer_halves.py).  Two numbers per tensor, both against float64: max|a - t| / max|t| over the
tensor ("whole") and the same per slice with the worst slice reported ("slice": per image for maps, mu, rstd and h; per head for lse; per
head-column block for qkv and att; per output row for weights and their gradients, i.e. per entry for vectors).  A slice whose truth is
identically zero must be identically zero.  Either number must stay within  K x (the float32 oracle's same number) + floor,  floor = one
fp32 ulp of the (worst) slice's largest magnitude; for the gradients that are sums over the tokens (LayerNorm weight and bias, the three
biases) the floor is one ulp of the sum of the magnitudes of the terms ("mag.g.*" of the restatement).  The caps of
tests/test_gpu_swinir.py (5e-5 / 2e-4 / 3e-4) stay on the whole-tensor numbers of y / dx / gradients.

K.  Every run prints  ``halves <run> <tensor> whole hip/o32 ratio slice hip/o32 ratio``  before it asserts, ratio = max(0, hip - floor)
/ oracle32; K = twice the worst measured ratio, rounded up.  Measured on the MI355X (each cell: the larger of the whole-tensor and the
worst-slice ratio; runs a-C-heads-ws-shift-B-H-W and m-C-hidden-B-H-W; g.ln = LayerNorm, [q] / [v] = the q / v part of the vector;
sat = saturated softmax, zv = zero-variance pixels):
    attention half         mu   rstd    qkv    lse    att      y     dx g.ln.w g.ln.b g.qkv.w g.qkv.b[q] g.qkv.b[v] g.proj.w g.proj.b
    a-12-4-1-0-2-3-5     0.00   0.00   0.72   0.73   0.72   0.05   0.25   0.00   0.00  0.79[v]        -       0.00     0.50     0.00
    a-8-2-2-1-3-2-2      0.64   0.00   0.11   0.11   0.70   0.01   0.19   0.27   0.30    0.50      0.00       1.11     0.49     0.00
    a-36-1-3-2-1-6-9     0.00   0.00   1.32   0.09   0.68   0.78   0.30   0.74   0.00    1.29      0.14       0.30     0.69     0.00
    a-132-4-5-3-1-5-10   0.30   0.56   0.90   0.40   0.76   0.61   1.60   1.04   0.71    0.90      0.42       0.65     0.95     0.00
    a-96-2-6-5-1-12-6    0.00   0.38   0.76   0.38   1.02   0.29   1.56   2.36   1.00    0.79      0.38       1.03     1.07     0.00
    a-56-2-7-3-2-7-14    0.21   0.45   0.84   0.31   0.81   0.75   0.84   0.79   0.41    0.94      0.00       0.75     0.89     0.00
    a-180-6-8-1-1-8-16   0.00   0.23   0.84   0.66   0.87   0.43   0.98   0.65   1.01    1.52      0.90       1.04     0.90     0.00
    a-64-1-8-7-1-16-8    0.00   0.34   0.71   0.11   0.76   0.64   1.12   0.92   0.69    1.29      0.17       0.99     1.24     0.00
    sat-ws7              0.00   0.00   0.61   1.04   1.07   0.96   0.56   4.90   2.17    0.69      0.80       0.67     0.00     0.00
    sat-ws3              0.34   0.00   0.46   0.35   1.34   1.96   0.73   1.49   0.93    0.96      2.20       0.00     0.00     0.00
    zv-attn              0.00   0.00   0.99   0.95   0.98   0.97   0.98   0.68   0.43    1.22      0.53       2.88     0.93     0.00
    MLP half               mu   rstd      h      y     dx g.ln.w g.ln.b g.fc1.w g.fc1.b g.fc2.w g.fc2.b
    m-4-8-1-1-1          0.75   0.00   0.00   0.00   0.00   0.90   0.21    1.44    1.39    0.00    0.00
    m-12-24-2-3-5        0.45   0.00   0.41   0.30   0.55   0.21   0.35    1.11    0.00    0.48    0.00
    m-20-52-1-7-9        0.00   0.13   0.98   0.26   0.20   0.00   0.00    1.12    0.00    0.60    0.00
    m-16-64-2-4-3        0.00   0.10   0.31   0.09   0.31   0.44   0.00    1.25    0.00    0.69    0.00
    m-180-360-1-4-6      0.00   0.00   0.81   1.55   0.68   0.69   0.66    1.29    0.25    0.82    0.69
    zv-mlp               0.00   0.00   0.00   0.00   0.00   0.01   0.00    0.03    0.00    0.03    0.00
    gelu-tails           0.00   0.00   0.41   1.27   0.53   0.09   0.00    0.59    0.00    1.00    0.00
The worst is 4.90 (sat-ws7, one entry of the LayerNorm weight gradient), so K = 10.  Without the two saturated runs the worst is 2.88 and
K would be 6, the K of the MDTA / GDFN file; the saturated runs sit higher for the reason given under KEY-BIAS GRADIENT below (a rounding
residue in dS that plain softmax autograd does not have), and 4.90 against 2.88 is no outlier of the kind that file's d temperature was
(7.94 against 2.82), so K follows the rule and no tensor has a K of its own.  zv-mlp: the float32 oracle itself is off by 2e-5 to 5e-5
there (x - mu of an all-equal pixel is the rounding of mu, times rstd = 316), the kernels are not.
img_affine: y within 0.50 ulp at r = 1 and 0.95 ulp at r = 255, dx within 0.50 ulp.

SINGLE-TOKEN WINDOWS (ws = 1), a statement that does not hold as an exact zero.  With one key P = 1 whatever the score, so dS = P (dP - D)
is zero in exact arithmetic, in float64 and in the float32 oracle: the q and k parts of d qkv.weight / d qkv.bias are identically zero
there.  The kernel forms dP = dO . v on the MFMA and D = dO . O by a wave reduction -- the same hd products in two summation orders -- so
its dS is a rounding residue, |dS| <= 2 hd 2^-24 sum_d |dO_d v_d|, not zero.  That is noise of the size the softmax rows of every larger
window carry in the same place (sum_j dS_ij = 0 holds there to the same residue), not a defect; the q and k parts of this run are therefore
held to that derived bound (test_single_token_window; measured: 0.06 of it on the bias, 0.07 on the weight) instead of to an exact zero,
and its v part to the measure.

KEY-BIAS GRADIENT.  d qkv.bias[C:2C] is zero in exact arithmetic (a constant added to every key moves each score row by a constant);
test_key_bias_gradient holds every entry to K ulp of the sum of magnitudes of the rows it column-sums.  Measured, worst |g| / ulp(sum|dk
rows|) (max|g| next to its floor): 0.81 (7.5e-08 / 2.4e-07), 1.34 (7.2e-07 / 9.5e-07), 2.12 (8.0e-07 / 9.5e-07), 2.19 (1.0e-06 / 9.5e-07),
1.31 (2.1e-06 / 1.9e-06), 2.75 (1.8e-06 / 1.9e-06), 2.69 (1.4e-06 / 9.5e-07) in the seven cases with ws > 1, 1.07 in zv-attn; the float32
oracle leaves 0.5 to 1.25.
FINDING: in the saturated runs that floor does not hold -- 8.60 (sat-ws7: max|g| 7.9e-05, floor 1.5e-05) and 17.12 (sat-ws3: 3.3e-05, 3.8e-06)
ulp of sum|dk rows|, where the float32 oracle leaves 0.5 and 1.0.  The cause is the measure and the order of two sums, not a lost digit:
in a one-hot row dS at the hot key is P (dP - D) with D = dP in exact arithmetic.  torch forms D = sum_j P_j dP_j from the same dP, so the
difference is an exact 0; the kernel forms D = dO . O by a wave reduction and dP = dO . v on the MFMA, so the difference is the residue of the
single-token case, 2^-24 of sum_d |dO_d v_d|, while the rows of dk -- and with them the floor -- have all but vanished.  What cancels in
d k-bias is sum_i sum_m P (|dP| + |D|) scale |q| (cancelled_magnitude in the CPU file), 25 to 110 times sum|dk rows| in these two runs and 2.6
to 12 times elsewhere; against one ulp of THAT the residues are 0.16 and 0.27, and the saturated runs are held to K ulp of it.  The eight
attention cases and zv-attn keep the floor as stated.  No kernel change: y, dx and every gradient of the saturated runs are inside the
measure with the same K.

SATURATED SOFTMAX.  lse is fp32 and the backward's P = exp(S - lse) inherits its rounding, a relative error of up to 2^-24 |lse| that plain
softmax autograd does not have; for dx and the gradients of the two saturated runs the floor gains 2^-24 max|lse| (derived, K unchanged,
caps unchanged).  Measured, HIP / oracle32 next to that term: sat-ws7 (max|lse| 195.3, term 1.16e-05) dx 1.61e-05 / 8.8e-06, d qkv.weight
1.90e-05 / 1.31e-05, d norm1.weight 1.12e-05 / 7.7e-06, d norm1.bias 1.35e-05 / 9.9e-06; sat-ws3 (136.3, 8.1e-06) dx 1.34e-05 / 7.2e-06,
d qkv.weight 1.04e-05 / 8.6e-06.  Every whole-tensor number is within twice the oracle's own error, term or no term; the worst slice number
is the 4.90 of the table (one entry of d norm1.weight: 8.9e-04 against 1.7e-04 of an entry that is itself a nearly cancelled sum).  Nothing
needed more than the term, and swin.hip is unchanged.

SENSITIVITY (scratch builds of swin.hip, not committed; each run once).  Scale 1 / sqrt(DP) instead of 1 / sqrt(hd): test_attn_stages fails
in the seven cases with hd not in {32, 64} and passes at hd = 64; test_single_token_window (lse), both saturated runs and zv-attn fail; the
old block tests catch it too (test_block_golden x 4, test_tiny_net_golden, test_block_vs_restatement_head_dims: y off by 1e-2 to 4e-1).
``j < g.N`` dropped from the backward's P: nothing fails, old or new, and by reading nothing can -- pad columns of P / dS meet zero rows of K
in dQ, and rows j >= N of dK / dV are never written; the mask is redundant with the zero padding of the operands (it would matter only
where exp(-lse) overflows, lse < -88, on an odd N).  The mask that does matter is the forward's: with ``lane < g.NP`` for ``lane < g.N`` in
the row softmax (the pad keys enter with score 0) test_attn_stages fails in the six cases with N not in {32, 64} and passes at ws = 8,
test_single_token_window, zv-attn and six key-bias cases fail, the saturated runs do not notice (as the CPU table says: e^(0 - max) is
nothing there); of the old tests the ws = 4 and ws = 2 blocks catch it, the ws = 8 ones cannot.  The ``py >= g.H`` wrap removed reads out of bounds and was not run: the CPU table
shows every shifted case telling a clamped map from a wrapped one on lse, att, y, dx and six gradients."""
import math

import numpy as np
import pytest
import torch

import tests.test_swin_restatement_cpu as C
from dcpt_amd.keyed_init import keyed_input
from kernel_trace import kernel_trace

pytestmark = pytest.mark.gpu
K = C.K


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


# ---- the HIP side: one run of a half, kept for every test that looks at it ----------------------------------------------------------------
_HIP = {}


def hip_run(dev, run):
    """-> ({stage / y / dx / g.*: CPU tensor}, kernel trace, the no-grad forward's y)"""
    if run in _HIP:
        return _HIP[run]
    from dcpt_amd import functional as DF

    half, case, _ = C.RUNS[run]
    x, dy, P = C.inputs(run)
    keys = C.ATTN_KEYS if half == "attn" else C.MLP_KEYS
    Pg = {k: P[k].clone().to(dev).requires_grad_(True) for k in keys}
    xg = x.clone().to(dev).requires_grad_(True)
    call = (lambda x_: DF.swin_attn(x_, *[Pg[k] for k in keys], *case[1:4])) if half == "attn" else (lambda x_: DF.swin_mlp(x_, *[Pg[k] for k in keys]))
    with kernel_trace() as tr:
        y = call(xg)
        saved = [t.detach().cpu() for t in y.grad_fn.saved_tensors]
        y.backward(dy.to(dev))
        torch.cuda.synchronize()
    out = dict(mu=saved[1][0], rstd=saved[1][1])
    if half == "attn":   # _SwinAttnFn.forward: save_for_backward(x, stats, qkv, att, lse, *parameters)
        out.update(qkv=saved[2], att=saved[3], lse=saved[4])
    else:                # _SwinMlpFn.forward: save_for_backward(x, stats, h, *parameters)
        out.update(h=saved[2])
    out.update(y=y.detach().cpu(), dx=xg.grad.cpu())
    out.update({"g." + k: p.grad.cpu() for k, p in Pg.items()})
    with torch.no_grad():   # saved = NULL: the intermediates live in the workspace
        lean = call(x.clone().to(dev)).cpu()
    _HIP[run] = (out, tr, lean)
    return _HIP[run]


def judge(run, hip, t64, o32):
    """print every figure, then assert them all at once"""
    bad = []
    for name, (wa, sa), (wo, so), (fw, fs), cap in C.judged(run, hip, t64, o32):
        rw = max(0.0, wa - fw) / wo if wo > 0 else (0.0 if wa <= fw else math.inf)
        rs = max(0.0, sa - fs) / so if so > 0 else (0.0 if sa <= fs else math.inf)
        print(f"halves {run} {name} whole {wa:.3e}/{wo:.3e} {rw:.2f} slice {sa:.3e}/{so:.3e} {rs:.2f}")
        if not wa <= K * wo + fw:
            bad.append(f"{name}: whole {wa:.3e} > {K} x {wo:.3e} + {fw:.1e}")
        if not sa <= K * so + fs:
            bad.append(f"{name}: worst slice {sa:.3e} > {K} x {so:.3e} + {fs:.1e}")
        if cap is not None and not wa <= cap:
            bad.append(f"{name}: whole {wa:.3e} > cap {cap:.1e}")
    assert not bad, f"{run}: " + "; ".join(bad)


def _finite(run, hip):
    for k, v in hip.items():
        assert bool(torch.isfinite(v).all()), f"{run} {k}: not finite"


PLAIN_ATTN = [r for r in C.ATTN_RUNS if C.RUNS[r][2] == "plain"]
PLAIN_MLP = [r for r in C.MLP_RUNS if C.RUNS[r][2] == "plain"]


@pytest.mark.parametrize("run", PLAIN_ATTN)
def test_attn_stages(dev, run):
    hip, _, _ = hip_run(dev, run)
    _finite(run, hip)
    judge(run, hip, *C.refs(run))


@pytest.mark.parametrize("run", PLAIN_MLP)
def test_mlp_stages(dev, run):
    hip, _, _ = hip_run(dev, run)
    _finite(run, hip)
    judge(run, hip, *C.refs(run))


def test_single_token_window(dev):
    """ws = 1: att is the v columns of the saved qkv bit for bit, lse is the scaled q . k, and the q and k parts of the qkv gradients -- zero
    in exact arithmetic -- are the rounding residue of dP - D at the most (the module docstring)"""
    run = PLAIN_ATTN[0]
    _, (Cc, heads, ws, shift, B, H, W), _ = C.RUNS[run]
    assert ws == 1
    hd, u = Cc // heads, 2.0 ** -24
    hip, _, _ = hip_run(dev, run)
    t64 = C.refs(run)[0]
    qkv = hip["qkv"]
    assert torch.equal(hip["att"], qkv[:, 2 * Cc:]), "one key: P = 1 and O = v exactly"
    scale = np.float32(1.0) / np.sqrt(np.float32(hd))
    q = (qkv[:, :Cc] * float(scale)).double().reshape(-1, heads, hd)      # the kernel rounds q * scale to fp32 before the product
    k = qkv[:, Cc:2 * Cc].double().reshape(-1, heads, hd)
    s = (q * k).sum(-1)
    assert bool(((hip["lse"].double() - s).abs() <= hd * u * (q * k).abs().sum(-1)).all()), "lse is not the scaled q . k"
    # the residue: |dS[m, h]| <= 2 hd u A[m, h], A = sum_d |dO_d v_d|;  dq = scale dS k, dk = scale dS q;  gradients sum them over the tokens
    x, dy, P = C.inputs(run)
    dO = (dy.double().permute(0, 2, 3, 1).reshape(-1, Cc) @ P["attn.proj.weight"].double()).reshape(-1, heads, hd)
    A = (dO * t64["qkv"][:, 2 * Cc:].reshape(-1, heads, hd)).abs().sum(-1, keepdim=True)
    other = torch.cat([t64["qkv"][:, Cc:2 * Cc], t64["qkv"][:, :Cc]], 1).abs()        # q's gradient carries k, k's carries q
    Ah = (A * hd ** -0.5).expand(-1, heads, hd).reshape(-1, Cc)
    rows = torch.cat([Ah, Ah], 1) * other                                              # (M, 2C): bound / (2 hd u) of |d qkv[m, c]|
    tol = 2 * hd * u * 1.01
    gb, gw = hip["g.attn.qkv.bias"][:2 * Cc].double(), hip["g.attn.qkv.weight"][:2 * Cc].double()
    bb, bw = rows.sum(0), rows.t() @ t64["xn"].abs()
    print(f"halves {run} residue: bias {float((gb.abs() / bb).max() / (2 * hd * u)):.2f}, weight {float((gw.abs() / bw).max() / (2 * hd * u)):.2f} of the bound")
    assert bool((t64["g.attn.qkv.bias"][:2 * Cc] == 0).all()) and bool((t64["g.attn.qkv.weight"][:2 * Cc] == 0).all())
    assert bool((gb.abs() <= tol * bb).all()) and bool((gw.abs() <= tol * bw).all())


@pytest.mark.parametrize("run", C.ATTN_RUNS)
def test_key_bias_gradient(dev, run):
    """|d qkv.bias[C:2C]| <= K ulp of the sum of magnitudes of the rows it column-sums (of what cancels in them, in the saturated runs: see
    the module docstring)"""
    Cc, ws = C.RUNS[run][1][0], C.RUNS[run][1][2]
    if ws == 1:
        return   # no rows to cancel: the derived residue bound of test_single_token_window holds this part
    hip, _, _ = hip_run(dev, run)
    g = hip["g.attn.qkv.bias"][Cc:2 * Cc].double().abs()
    floor = C.key_bias_floor(run)
    r = g / floor
    print(f"halves {run} key-bias: max|g| {float(g.max()):.3e}, floor {float(floor.max()):.3e}, worst |g| / ulp(mag) {float(r.max()):.2f}")
    assert bool((g <= K * floor).all()), f"{run}: worst key-bias residue is {float(r.max()):.2f} ulp of its magnitude sum"


@pytest.mark.parametrize("run", ["sat-ws7", "sat-ws3"])
def test_saturated_softmax(dev, run):
    """scores past +-60, max|lse| in [60, 200], a quarter of the rows one-hot to fp32 (asserted on the reference by the CPU file)"""
    hip, _, _ = hip_run(dev, run)
    _finite(run, hip)
    t64, o32 = C.refs(run)
    print(f"halves {run} max|lse| {float(t64['lse'].abs().max()):.1f}: the floors of dx and the gradients gain {C.lse_term(run, t64):.3e}")
    judge(run, hip, t64, o32)


@pytest.mark.parametrize("run", ["zv-attn", "zv-mlp"])
def test_zero_variance_pixels(dev, run):
    """three pixels whose channels are all equal (0, 0.7, -3.0): rstd = 1 / sqrt(1e-5) there, the largest gain the LayerNorm backward applies"""
    hip, _, _ = hip_run(dev, run)
    _finite(run, hip)
    judge(run, hip, *C.refs(run))


def test_gelu_tails(dev):
    """fc1 scaled so that h of the float64 reference spans at least [-8, 8]: gelu(h) is h or ~ -0 and gelu' 1 or 0 there"""
    hip, _, _ = hip_run(dev, "gelu-tails")
    _finite("gelu-tails", hip)
    judge("gelu-tails", hip, *C.refs("gelu-tails"))


@pytest.mark.parametrize("run", list(C.RUNS))
def test_lean_equals_full(dev, run):
    """the torch.no_grad() forward (saved = NULL, intermediates in the workspace) equals the grad-mode y bit for bit"""
    hip, _, lean = hip_run(dev, run)
    assert torch.equal(lean, hip["y"])


@pytest.mark.parametrize("run", C.ATTN_RUNS)
def test_kernel_trace(dev, run):
    _, tr, _ = hip_run(dev, run)
    assert tr["swin_wattn_fwd"] == 1 and tr["swin_wattn_bwd"] == 1, tr.counts


# ---- image affine -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1.0, 255.0])
@pytest.mark.parametrize("B,Cc,HW", [(2, 3, 5), (1, 1, 7)])
def test_img_affine(dev, B, Cc, HW, r):
    """(x - mean) r and x / r + mean and their backward (dy r, dy / r) within 1.5 fp32 ulp of the float64 result: two roundings each"""
    from dcpt_amd import functional as DF

    tag = f"swh.aff{B}{Cc}{HW}"
    mean = keyed_input(tag + ".m", (Cc,), lo=0.1, hi=0.9)
    dy = keyed_input(tag + ".dy", (B, Cc, HW, 1), lo=-1.0, hi=1.0)
    md = mean.double().reshape(1, Cc, 1, 1)
    for direction in (0, 1):
        x = keyed_input(tag + f".x{direction}", (B, Cc, HW, 1), lo=0.0, hi=(1.0 if direction == 0 else r))
        xg = x.to(dev).requires_grad_(True)
        y = DF.img_affine(xg, mean.to(dev), r, direction)
        y.backward(dy.to(dev))
        ty = (x.double() - md) * r if direction == 0 else x.double() / r + md
        tdx = dy.double() * r if direction == 0 else dy.double() / r
        for name, a, t in (("y", y.detach().cpu(), ty), ("dx", xg.grad.cpu(), tdx)):
            ulp = torch.from_numpy(np.spacing(t.abs().float().numpy())).double()
            e = float(((a.double() - t).abs() / ulp).max())
            print(f"img_affine B{B} C{Cc} HW{HW} r{r} dir{direction} {name}: {e:.2f} ulp")
            assert e <= 1.5, f"dir {direction} {name}: {e:.2f} ulp"
