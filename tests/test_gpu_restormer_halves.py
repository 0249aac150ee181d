"""The fp32 MDTA and GDFN halves (dcpt_mdta_fwd / _bwd, dcpt_gdfn_fwd / _bwd; DF.mdta / DF.gdfn) stage by stage against float64.

Each case calls one half directly in the "full" save mode, reads every tensor the forward keeps for the backward off ``y.grad_fn`` and
compares it, then y, dx and every parameter gradient, with the oracle (oracle.restormer_oracle / promptir_oracle ``layernorm`` +
``attention`` / ``feedforward`` + the residual) evaluated twice on the CPU from the same fp32 inputs: in float64 (the truth) and in
float32 (the yardstick).  The stage values come from a line-by-line restatement of the oracle below (``mdta_ref`` / ``gdfn_ref``) whose
end result is asserted bit-identical to the oracle function itself.

ERROR MEASURE.  Two numbers per tensor, both against float64: the tensor's max|a - t| / max|t| ("whole"), and the same ratio per slice
along the tensor's leading structural axis with the worst slice reported ("slice": per head for ghat / attn / attnT / temperature, per
output channel for weights and their gradients, per channel for nrm, per image for maps and for mu / rstd).  A slice whose truth is
identically zero must be identically zero.  Either number must stay within  K x (the float32 CPU oracle's same number) + floor,  floor =
one fp32 ulp of the (worst) slice's largest magnitude; on top, the project's caps on the whole-tensor number of y / dx / gradients stay
as an outer bound (5e-5 / 2e-4 / 3e-4 ReLU forms, 5e-5 / 3e-4 / 5e-4 softmax forms).

K.  Measured on the MI355X (this file with ``-s``: every case prints  ``halves <case> <tensor> whole hip/o32 ratio, slice ...``  before it
asserts), ratio = max(0, hip - floor) / oracle32.  The kernels sum in another order than the CPU (split-K Gram slabs, per-block partials,
MFMA k-order), so ratios somewhat above 1 are expected; K = twice the worst measured ratio, rounded up.
Measured (each cell: the larger of the whole-tensor and the worst-slice ratio; g.ln = norm weight, g.ln.bi = norm bias, g.p_in / g.p_out =
project_in / project_out, g.dw = depthwise taps; zv = zero-variance pixels, -0 / -1 = eps 1e-6 / 1e-5):
    MDTA
                                    mu   rstd     xn   qkv1    qkv    nrm   ghat   attn  attnT out_at      y     dx   g.ln g.ln.b  g.qkv   g.dw g.p_ou g.temp
    relu-WithBias-c12h1-2x5x7     0.00   0.00   0.53   0.46   0.51   0.47   0.45   0.63   0.63   0.53   0.00   0.75   1.05   1.83   0.98   1.37   1.31   0.00
    relu-BiasFree-c36h3-1x9x4     0.18   0.22   0.28   0.44   0.37   0.45   1.29   1.27   1.27   0.49   0.44   0.47   0.83      -   0.95   1.08   0.76   0.08
    relu-WithBias-c16h4-3x4x6     0.00   0.06   0.38   0.52   0.46   0.21   0.72   0.62   0.62   0.54   0.03   1.01   1.94   0.59   0.78   0.76   0.89   0.00
    relu-BiasFree-c48h2-1x24x23   0.00   0.00   0.56   0.76   0.65   0.19   0.91   0.73   0.73   0.60   0.38   0.90   0.95      -   0.84   0.69   0.98   2.74
    sm-WithBias-c68h1-1x6x5       0.00   0.79   0.72   0.61   0.51   0.25   0.65   0.56   0.56   0.99   0.00   0.00   0.63   0.98   0.96   1.07   0.90   0.00
    sm-BiasFree-c132h1-2x3x5      0.00   0.53   0.79   1.11   0.97   0.73   1.20   0.68   0.68   1.32   0.26   0.00   0.81      -   1.11   0.91   1.04   0.00
    sm-WithBias-c196h1-1x4x4      0.87   0.00   0.31   1.14   1.08   1.97   0.87   0.84   0.84   1.37   0.00   0.16   1.29   1.99   1.75   2.75   1.58   0.00
    sm-BiasFree-c40h2-2x5x3       0.00   0.10   0.28   0.73   0.42   0.85   0.94   0.56   0.56   0.55   0.34   0.00   0.51      -   0.86   0.67   1.32   0.00
    dead-relu                     0.00   0.00   0.37   0.51   0.35   0.20   0.42   0.89   0.89   0.60   0.53   0.85   2.82   1.54   1.01   0.93   0.85   0.00
    dead-sm                       0.00   0.00   0.02   0.48   1.24   0.52   0.67   0.27   0.27   0.61   0.24   0.78   0.87      -   0.81   0.81   0.68   0.00
    faint-relu                    0.00   0.17   0.32   0.65   0.15   0.00   0.48   0.47   0.47   0.55   0.29   0.61   1.97      -   0.87   0.65   1.26   0.00
    faint-sm                      0.09   0.00   0.26   0.19   0.40   0.13   0.85   0.47   0.47   1.03   0.31   0.92   1.61   0.47   1.66   1.05   1.06   0.00
    zv-mdta-WithBias-0            0.00   0.00   0.07   0.76   0.44   0.32   0.74   0.70   0.70   0.42   0.43   0.82   0.82   1.89   1.09   0.85   0.40   0.89
    zv-mdta-WithBias-1            0.00   0.00   0.45   0.67   0.38   0.00   0.60   0.00   0.00   0.39   0.00   1.33   1.55   0.50   0.79   0.93   0.56   0.00
    zv-mdta-BiasFree-0            0.00   0.00   0.00   0.13   0.82   0.76   0.59   0.27   0.27   0.72   1.06   0.62   0.84      -   1.32   0.87   0.97   1.28
    zv-mdta-BiasFree-1            0.00   0.00   0.35   0.84   0.83   2.27   1.08   0.29   0.29   0.49   0.87   1.26   1.70      -   1.15   1.22   0.90   0.00
    temp-relu                     0.00   0.00   0.46   0.49   0.10   0.00   0.55   0.68   0.68   0.72   0.24   1.20   0.79      -   1.51   1.53   2.45   1.86
    temp-sm                       0.00   0.00   0.25   0.30   0.51   0.29   0.54   0.76   0.76   0.93   0.74   0.79   1.01   0.86   1.00   1.00   1.22   0.24
    GDFN
                              mu   rstd     xn    u.1    u.2      t      y     dx   g.ln g.ln.b g.p_in   g.dw g.p_ou
    gdfn-WithBias-c56h148   0.00   0.32   0.36   0.58   0.50   0.75   1.01   0.60   1.40   1.62   0.96   0.64   0.82
    gdfn-BiasFree-c12h31    0.21   0.00   0.12   0.78   0.15   1.12   0.96   1.04   0.63      -   1.03   0.83   0.80
    gdfn-WithBias-c16h42    0.00   0.00   0.05   0.62   0.63   0.13   0.51   0.49   0.57   1.45   0.85   0.72   1.37
    gdfn-BiasFree-c8h21     0.00   0.00   0.20   0.09   0.11   0.08   0.61   0.48   1.19      -   0.94   0.58   0.61
    gdfn-BiasFree-c16h64    0.09   0.15   0.48   0.45   0.43   0.54   0.55   0.83   1.56      -   0.85   0.56   1.29
    zv-gdfn-WithBias-0      0.00   0.00   0.37   0.53   0.57   0.27   0.45   0.49   0.82   1.80   0.82   1.09   0.70
    zv-gdfn-WithBias-1      0.00   0.00   0.31   0.45   0.48   0.41   0.50   1.92   0.94   1.49   0.89   0.71   0.88
    zv-gdfn-BiasFree-0      0.00   0.00   0.00   0.98   1.00   0.86   0.95   0.67   2.19      -   0.77   0.80   0.61
    zv-gdfn-BiasFree-1      0.00   0.00   0.24   0.46   0.53   0.81   0.45   1.30   1.41      -   0.42   0.90   0.74
    gelu-tails              0.00   0.00   0.52   0.43   0.43   0.55   0.86   0.75   1.89   1.55   0.94   1.02   1.00
The worst is 2.82 (dead-relu, norm weight gradient, one channel), so K = 6.
FINDING: d temperature.  With the floor as above its ratio reached 7.94 (relu-BiasFree-c48h2: HIP 4.7e-7, oracle32 4.8e-8 of the value)
and 5.72 (sm-BiasFree-c40h2), i.e. K = 16.  The cause is the measure, not the kernel: d temperature[h] is ONE number per head, the sum of
B ch^2 products dpre * ghat of both signs (sum|terms| / |sum| = 3 ... 85 in these cases), so an fp32 error of a few ulp of the RESULT is
a fraction of an ulp of what was summed, and the float32 oracle's own error on a single number is one draw that can land anywhere below
that (0.4 ulp in the 7.94 case).  Its floor is therefore one fp32 ulp of sum|dpre * ghat| over the head (from the float64 reference,
``mag.g.attn.temperature``) instead of one ulp of the sum itself; the errors stay relative to the value, K is the same, and the cap of the
whole-tensor number still applies.  The table above is with that floor.

DISCONTINUITY.  ReLU attention flips a mask where temperature * ghat is within rounding of 0, so every ReLU case asserts on the float64
reference that min|t * ghat| >= 1e-4 max|t * ghat| over ALL entries that are not zero by construction (the row / column of a dead
channel, a head whose temperature is 0) -- no other entry is excluded.  The seeds below were chosen on the CPU so that this holds.

DEPTHWISE PATHS.  Every case asserts its depthwise kernel families by trace tag.  MDTA: the forward is always the register kernel
("dw.reg_plain_fwd_f32"); the backward is the row ring ("dw.ring_plain_bwd_f32") when 3C % 8 == 0 and the register kernel
("dw.reg_bwd_f32") otherwise, i.e. at every width with C % 8 == 4.  GDFN: the padded hidden width hp is a multiple of 4, so 2 hp % 8 == 0,
hp * 4 bytes % 16 == 0 and hp % 2 == 0 always hold and dwf_ring / dwb_ring (restormer.hip) can only refuse B > 65535 -- which the register
forms refuse as well (DCPT_CHECK_ARG B <= 65535 in launch_dw_gelu_fwd / _gelu_bwd_a / _generic_bwd).  So "dw.reg_gelu_fwd_f32",
"dw.reg_gelu_bwd_a_f32" and GDFN's call of "dw.reg_bwd_f32" are unreachable from any legal fp32 shape: every GDFN case here (pad 0, 1, 2, 3;
one and several ring row blocks; both save modes) ran "dw.ring_gelu_fwd_f32" / "dw.ring_gelu_bwd_f32" and asserts that none of the three
register families ran.

A channel of q or k whose L2 norm is EXACTLY zero does not exercise the ``n > NORM_EPS`` guard of attn_bwd_kernel: the sum the guard
protects is then exactly zero as well (-0 / n^2).  test_mdta_faint_channel therefore adds a channel whose norm is 5e-13 -- below
F.normalize's eps but not zero -- where the guard decides between the right gradient and one that is off by percent.

A NEGATIVE temperature does not give a dead head under ReLU: relu(t ghat) is positive wherever ghat is negative, in the reference as in the
kernels.  Only the head with t = 0 is all zero (test_mdta_temperature_relu).  Zero-variance pixels: LN(x) of a pixel whose channels are all
equal has rstd = 1 / sqrt(eps), 1000 or 316; rstd and xn are stages, and dx around those pixels is under the per-image number."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import keyed_input, keyed_tensor
from kernel_trace import kernel_trace
from oracle import promptir_oracle as PO
from oracle import restormer_oracle as RO

pytestmark = pytest.mark.gpu

K = 6    # twice the worst measured HIP / oracle32 ratio (2.82), rounded up: see the module docstring
CAPS = {False: (5e-5, 2e-4, 3e-4), True: (5e-5, 3e-4, 5e-4)}   # softmax? -> caps on y / dx / parameter gradients (whole-tensor number)
MARGIN = 1e-4
NORM_EPS = np.float32(1e-12)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


# ---- the error measure ------------------------------------------------------------------------------------------------------------
def per_image(v):
    return v.reshape(v.shape[0], -1)


def per_row(v):          # output channel of a weight / head of the temperature
    return v.reshape(v.shape[0], -1)


def per_head(v):         # [B][heads][ch][ch]
    return v.permute(1, 0, 2, 3).reshape(v.shape[1], -1)


def per_channel(v):      # nrm [B][2C]
    return v.t()


def _ulp_rel(m, of=None):
    """one fp32 ulp of the magnitude ``of`` (default: m itself) relative to m"""
    m, of = float(m), float(m if of is None else of)
    return float(np.spacing(np.float32(of))) / m if m > 0 else 0.0


def _numbers(a, t, sl, mag=None):
    """(whole, floor of whole, worst slice, floor of that slice), all relative to the largest magnitude of the truth.  ``mag``: per slice,
    the magnitude the floor's ulp is taken of where that is not the slice's own largest value (the terms of a sum)"""
    a2, t2 = sl(a.double()), sl(t.double())
    assert a2.shape == t2.shape, (a2.shape, t2.shape)
    d = (a2 - t2).abs()
    dm, tm = d.amax(1), t2.abs().amax(1)
    mag = tm if mag is None else mag.double().flatten()
    assert mag.shape == tm.shape and bool((mag >= tm).all())
    e = torch.where(tm > 0, dm / tm.clamp_min(1e-300), torch.where(dm == 0, torch.zeros_like(dm), torch.full_like(dm, math.inf)))
    i = int(e.argmax())
    wm = float(tm.max())
    whole = float(dm.max()) / wm if wm > 0 else (0.0 if float(dm.max()) == 0 else math.inf)
    return whole, _ulp_rel(wm, mag.max()), float(e[i]), _ulp_rel(tm[i], mag[i])


class Ledger:
    """collects (tensor, HIP numbers, oracle32 numbers) of one case; judge() prints every figure, then asserts them all at once"""

    def __init__(self, case, softmax=False):
        self.case, self.rows, self.caps = case, [], CAPS[softmax]

    def add(self, name, a, o, t, sl, cap=None, mag=None):
        a = a.detach().cpu()
        assert bool(torch.isfinite(a).all()), f"{self.case} {name}: not finite"
        assert tuple(a.shape) == tuple(t.shape), (name, a.shape, t.shape)
        self.rows.append((name, _numbers(a, t, sl, mag), _numbers(o, t, sl, mag), cap))

    def results(self, hip, o32, t64, maps=("y", "dx")):
        for k in t64:
            if not (k in maps or k.startswith("g.")):
                continue
            cap = self.caps[0] if k == "y" else self.caps[1] if k == "dx" else self.caps[2]
            self.add(k, hip[k], o32[k], t64[k], per_image if k in maps else per_row, cap, t64.get("mag." + k))

    def judge(self):
        bad = []
        for name, (wa, fw, sa, fs), (wo, _, so, _), cap in self.rows:
            rw = max(0.0, wa - fw) / wo if wo > 0 else (0.0 if wa <= fw else math.inf)
            rs = max(0.0, sa - fs) / so if so > 0 else (0.0 if sa <= fs else math.inf)
            print(f"halves {self.case} {name} whole {wa:.3e}/{wo:.3e} {rw:.2f} slice {sa:.3e}/{so:.3e} {rs:.2f}")
            if not wa <= K * wo + fw:
                bad.append(f"{name}: whole {wa:.3e} > {K} x {wo:.3e} + {fw:.1e}")
            if not sa <= K * so + fs:
                bad.append(f"{name}: worst slice {sa:.3e} > {K} x {so:.3e} + {fs:.1e}")
            if cap is not None and not wa <= cap:
                bad.append(f"{name}: whole {wa:.3e} > cap {cap:.1e}")
        assert not bad, f"{self.case}: " + "; ".join(bad)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _maps(tag, C, B, H, W, seed):
    """x with a per-channel offset (the BiasFree numerator is not centred; mu is a stage) and the output gradient"""
    x = keyed_input(tag + ".x", (B, C, H, W), seed, lo=-2.0, hi=2.0) + keyed_input(tag + ".xo", (1, C, 1, 1), seed, lo=-1.0, hi=1.0)
    return x, keyed_input(tag + ".dy", (B, C, H, W), seed, lo=-1.0, hi=1.0)


def mdta_inputs(tag, lnt, C, heads, B, H, W, seed=0):
    shapes = {"norm1.body.weight": (C,), "norm1.body.bias": (C,), "attn.qkv.weight": (3 * C, C, 1, 1),
              "attn.qkv_dwconv.weight": (3 * C, 1, 3, 3), "attn.project_out.weight": (C, C, 1, 1), "attn.temperature": (heads, 1, 1)}
    if lnt == "BiasFree":
        del shapes["norm1.body.bias"]
    P = {k: keyed_tensor(f"{tag}.{k}", s, seed) for k, s in shapes.items()}
    return (*_maps(tag, C, B, H, W, seed), P)


def gdfn_inputs(tag, lnt, C, hidden, B, H, W, seed=0):
    shapes = {"norm2.body.weight": (C,), "norm2.body.bias": (C,), "ffn.project_in.weight": (2 * hidden, C, 1, 1),
              "ffn.dwconv.weight": (2 * hidden, 1, 3, 3), "ffn.project_out.weight": (C, hidden, 1, 1)}
    if lnt == "BiasFree":
        del shapes["norm2.body.bias"]
    P = {k: keyed_tensor(f"{tag}.{k}", s, seed) for k, s in shapes.items()}
    return (*_maps(tag, C, B, H, W, seed), P)


# ---- references: the oracle for the results, its restatement for the stages -------------------------------------------------------------
def _ln_stats(x, eps):
    b, c, h, w = x.shape
    t = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
    return t.mean(-1), 1.0 / torch.sqrt(t.var(-1, unbiased=False) + eps)


def _results(x, y, dy, P):
    y.backward(dy)
    out = {"y": y.detach(), "dx": x.grad}
    out.update({"g." + k: p.grad for k, p in P.items()})
    return out


def mdta_ref(x, dy, P, dt, eps_1e5=False, softmax=False):
    LN = (PO if eps_1e5 else RO).layernorm
    ATT = (PO if softmax else RO).attention
    P = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in P.items()}
    x = x.detach().clone().to(dt).requires_grad_(True)
    out = _results(x, x + ATT(LN(x, P, "norm1."), P, "attn."), dy.to(dt), P)
    with torch.no_grad():
        b, c, h, w = x.shape
        heads = P["attn.temperature"].shape[0]
        out["mu"], out["rstd"] = _ln_stats(x, 1e-5 if eps_1e5 else 1e-6)
        xn = out["xn"] = LN(x, P, "norm1.")
        out["qkv1"] = F.conv2d(xn, P["attn.qkv.weight"])
        out["qkv"] = F.conv2d(out["qkv1"], P["attn.qkv_dwconv.weight"], padding=1, groups=3 * c)
        q, k, v = (t.reshape(b, heads, c // heads, h * w) for t in out["qkv"].chunk(3, dim=1))
        out["nrm"] = torch.cat([q.norm(dim=-1).reshape(b, c), k.norm(dim=-1).reshape(b, c)], 1).clamp_min(1e-12)
        out["ghat"] = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
        pre = out["pre"] = out["ghat"] * P["attn.temperature"]
        out["attn"] = pre.softmax(dim=-1) if softmax else F.relu(pre)
        out["attnT"] = out["attn"].transpose(-2, -1)
        out["out_att"] = (out["attn"] @ v).reshape(b, c, h, w)
        assert torch.equal(F.conv2d(out["out_att"], P["attn.project_out.weight"]), ATT(xn, P, "attn.")), "the staged copy left the oracle"
    # d temperature[h] = sum over (image, i, j) of dpre * ghat: the magnitude of what that sum adds up, for the floor of its bound
    pl = pre.clone().requires_grad_(True)
    a = pl.softmax(dim=-1) if softmax else F.relu(pl)
    F.conv2d((a @ v).reshape(b, c, h, w), P["attn.project_out.weight"].detach()).backward(dy.to(dt))
    terms = pl.grad * out["ghat"]
    assert torch.allclose(terms.sum((0, 2, 3)), out["g.attn.temperature"].flatten(), rtol=1e-4, atol=1e-30)
    out["mag.g.attn.temperature"] = terms.abs().sum((0, 2, 3))
    return out


def gdfn_ref(x, dy, P, dt, eps_1e5=False):
    LN = (PO if eps_1e5 else RO).layernorm
    P = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in P.items()}
    x = x.detach().clone().to(dt).requires_grad_(True)
    out = _results(x, x + RO.feedforward(LN(x, P, "norm2."), P, "ffn."), dy.to(dt), P)
    with torch.no_grad():
        out["mu"], out["rstd"] = _ln_stats(x, 1e-5 if eps_1e5 else 1e-6)
        xn = out["xn"] = LN(x, P, "norm2.")
        u = out["u"] = F.conv2d(xn, P["ffn.project_in.weight"])
        x1, x2 = F.conv2d(u, P["ffn.dwconv.weight"], padding=1, groups=u.shape[1]).chunk(2, dim=1)
        out["x1"] = x1
        out["t"] = F.gelu(x1) * x2
        assert torch.equal(F.conv2d(out["t"], P["ffn.project_out.weight"]), RO.feedforward(xn, P, "ffn.")), "the staged copy left the oracle"
    return out


def relu_margin(t64, zero_rows=(), zero_cols=(), zero_heads=()):
    """min / max of |temperature * ghat| of the float64 reference over every entry that is not zero by construction"""
    pre = t64["pre"].abs()
    keep = torch.ones_like(pre, dtype=torch.bool)
    for h, i in zero_rows:
        keep[:, h, i, :] = False
    for h, j in zero_cols:
        keep[:, h, :, j] = False
    for h in zero_heads:
        keep[:, h] = False
    assert bool((pre[~keep] == 0).all()), "an excluded entry is not zero"
    return float(pre[keep].min() / pre[keep].max())


# ---- the HIP side -------------------------------------------------------------------------------------------------------------------
def mdta_hip(dev, x, dy, P, heads, eps_1e5=False, softmax=False, mode="full"):
    from dcpt_amd import functional as DF

    Pg = {k: v.to(dev).requires_grad_(True) for k, v in P.items()}
    xg = x.to(dev).requires_grad_(True)
    prev = DF.set_restormer_save(mode)
    try:
        with kernel_trace() as tr:
            y = DF.mdta(xg, Pg["norm1.body.weight"], Pg.get("norm1.body.bias"), Pg["attn.qkv.weight"], Pg["attn.qkv_dwconv.weight"],
                        Pg["attn.project_out.weight"], Pg["attn.temperature"], heads, "norm1.body.bias" not in P, eps_1e5=eps_1e5,
                        softmax=softmax)
            out = {}
            if mode == "full":   # _MDTAFn.forward: save_for_backward(x, stats, qkv, nrm, att, qkv1, out_att, xn, *parameters)
                _, stats, qkv, nrm, att, qkv1, out_att, xn = (t.detach().cpu() for t in y.grad_fn.saved_tensors[:8])
                B = x.shape[0]
                out.update(mu=stats[0].reshape(B, -1), rstd=stats[1].reshape(B, -1), qkv=qkv, nrm=nrm, ghat=att[0], attn=att[1], attnT=att[2],
                           qkv1=qkv1, out_att=out_att, xn=xn)
            y.backward(dy.to(dev))
    finally:
        DF.set_restormer_save(prev)
    out.update(y=y.detach().cpu(), dx=xg.grad.cpu())
    out.update({"g." + k: p.grad.cpu() for k, p in Pg.items()})
    return out, tr


def gdfn_hip(dev, x, dy, P, eps_1e5=False, mode="full"):
    from dcpt_amd import functional as DF

    Pg = {k: v.to(dev).requires_grad_(True) for k, v in P.items()}
    xg = x.to(dev).requires_grad_(True)
    prev = DF.set_restormer_save(mode)
    try:
        with kernel_trace() as tr:
            y = DF.gdfn(xg, Pg["norm2.body.weight"], Pg.get("norm2.body.bias"), Pg["ffn.project_in.weight"], Pg["ffn.dwconv.weight"],
                        Pg["ffn.project_out.weight"], "norm2.body.bias" not in P, eps_1e5=eps_1e5)
            out = {}
            if mode == "full":   # _GDFNFn.forward: save_for_backward(x, stats, u, t, xn, *parameters); u [B][2 hp][H][W], t [B][hp][H][W]
                _, stats, u, t, xn = (s.detach().cpu() for s in y.grad_fn.saved_tensors[:5])
                B = x.shape[0]
                out.update(mu=stats[0].reshape(B, -1), rstd=stats[1].reshape(B, -1), u=u, t=t, xn=xn)
            y.backward(dy.to(dev))
    finally:
        DF.set_restormer_save(prev)
    out.update(y=y.detach().cpu(), dx=xg.grad.cpu())
    out.update({"g." + k: p.grad.cpu() for k, p in Pg.items()})
    return out, tr


MDTA_STAGES = (("mu", per_image), ("rstd", per_image), ("xn", per_image), ("qkv1", per_image), ("qkv", per_image), ("nrm", per_channel),
               ("ghat", per_head), ("attn", per_head), ("attnT", per_head), ("out_att", per_image))
MDTA_DW = {"generic": {"dw.reg_plain_fwd_f32": 1, "dw.reg_bwd_f32": 1}, "ring": {"dw.reg_plain_fwd_f32": 1, "dw.ring_plain_bwd_f32": 1}}
GDFN_DW = {"dw.ring_gelu_fwd_f32": 1, "dw.ring_gelu_bwd_f32": 1}


def mdta_case(dev, case, x, dy, P, heads, eps_1e5, softmax, path, zero=None):
    """one MDTA half in "full" mode: path, stages and results into a Ledger (not judged yet: the caller may add its own checks)"""
    t64, o32 = mdta_ref(x, dy, P, torch.float64, eps_1e5, softmax), mdta_ref(x, dy, P, torch.float32, eps_1e5, softmax)
    if not softmax:
        m = relu_margin(t64, **(zero or {}))
        assert m >= MARGIN, f"{case}: min|t ghat| is {m:.2e} of its max in the float64 reference: choose other inputs"
    hip, tr = mdta_hip(dev, x, dy, P, heads, eps_1e5, softmax)
    assert tr.families("dw.") == MDTA_DW[path], tr.counts
    assert torch.equal(hip["attnT"], hip["attn"].transpose(-2, -1)), "attnT is not the transpose of attn"
    led = Ledger(case, softmax)
    for name, sl in MDTA_STAGES:
        led.add(name, hip[name], o32[name], t64[name], sl)
    led.results(hip, o32, t64)
    return led, hip, t64, o32


def gdfn_case(dev, case, x, dy, P, eps_1e5=False):
    t64, o32 = gdfn_ref(x, dy, P, torch.float64, eps_1e5), gdfn_ref(x, dy, P, torch.float32, eps_1e5)
    hip, tr = gdfn_hip(dev, x, dy, P, eps_1e5)
    assert tr.families("dw.") == GDFN_DW, tr.counts   # none of dw.reg_gelu_fwd_f32 / dw.reg_gelu_bwd_a_f32 / dw.reg_bwd_f32
    hidden = P["ffn.project_out.weight"].shape[1]
    hp = (hidden + 3) // 4 * 4
    u, t = hip["u"], hip["t"]
    assert u.shape[1] == 2 * hp and t.shape[1] == hp
    for name, pad in (("u", u[:, hidden:hp]), ("u", u[:, hp + hidden:]), ("t", t[:, hidden:])):
        assert pad.numel() == (hp - hidden) * t.shape[0] * t.shape[2] * t.shape[3]
        assert bool((pad == 0).all()), f"{case}: a pad column of the saved {name} is not exactly zero"
    led = Ledger(case)
    for name in ("mu", "rstd", "xn"):
        led.add(name, hip[name], o32[name], t64[name], per_image)
    led.add("u.1", u[:, :hidden], o32["u"][:, :hidden], t64["u"][:, :hidden], per_image)
    led.add("u.2", u[:, hp:hp + hidden], o32["u"][:, hidden:], t64["u"][:, hidden:], per_image)
    led.add("t", t[:, :hidden], o32["t"], t64["t"], per_image)
    led.results(hip, o32, t64)
    return led, hip, t64, o32


# ---- the tables -------------------------------------------------------------------------------------------------------------------
#             LN          C   heads B  H   W  softmax  path      seed
MDTA_CASES = [("WithBias", 12, 1, 2, 5, 7, False, "generic", 0),      # smallest legal ch
              ("BiasFree", 36, 3, 1, 9, 4, False, "generic", 0),      # ch = 12, several heads
              ("WithBias", 16, 4, 3, 4, 6, False, "ring", 0),         # ch = 4
              ("BiasFree", 48, 2, 1, 24, 23, False, "ring", 9),       # P = 552: two Gram splits of 288 + 264 rows
              ("WithBias", 68, 1, 1, 6, 5, True, "generic", 0),       # ch = 68: second lane group of the softmax ragged
              ("BiasFree", 132, 1, 2, 3, 5, True, "generic", 0),      # ch = 132: third lane group ragged
              ("WithBias", 196, 1, 1, 4, 4, True, "generic", 0),      # ch = 196: fourth lane group ragged
              ("BiasFree", 40, 2, 2, 5, 3, True, "ring", 0)]          # ch = 20
#             LN          C   hidden B  H   W
GDFN_CASES = [("WithBias", 56, 148, 1, 7, 9),      # hp - hidden = 0: pack / unpack are the identity
              ("BiasFree", 12, 31, 1, 7, 9),       # 1
              ("WithBias", 16, 42, 1, 7, 9),       # 2
              ("BiasFree", 8, 21, 1, 7, 9),        # 3
              ("BiasFree", 16, 64, 3, 33, 17)]     # factor 4, no padding; several ring row blocks, odd W


def _mdta_id(c):
    return f"{'sm' if c[6] else 'relu'}-{c[0]}-c{c[1]}h{c[2]}-{c[3]}x{c[4]}x{c[5]}"


def _mdta_tag(c):
    return "hv.m" + _mdta_id(c)


@pytest.mark.parametrize("cfg", MDTA_CASES, ids=_mdta_id)
def test_mdta_stages(dev, cfg):
    lnt, C, heads, B, H, W, softmax, path, seed = cfg
    assert (3 * C % 8 == 0) == (path == "ring")
    x, dy, P = mdta_inputs(_mdta_tag(cfg), lnt, C, heads, B, H, W, seed)
    led, *_ = mdta_case(dev, _mdta_id(cfg), x, dy, P, heads, softmax, softmax, path)
    led.judge()


@pytest.mark.parametrize("cfg", GDFN_CASES, ids=lambda c: f"{c[0]}-c{c[1]}h{c[2]}-{c[3]}x{c[4]}x{c[5]}")
def test_gdfn_stages(dev, cfg):
    lnt, C, hidden, B, H, W = cfg
    assert hidden == int(C * 2.66) or (C, hidden) == (16, 64)
    tag = f"gdfn-{lnt}-c{C}h{hidden}"
    x, dy, P = gdfn_inputs("hv." + tag, lnt, C, hidden, B, H, W)
    led, *_ = gdfn_case(dev, tag, x, dy, P)
    led.judge()


def _same(a, b):
    for k in b:
        assert torch.equal(a[k], b[k]), f"{k} differs between the save modes"


def test_lean_equals_full(dev):
    """outputs and gradients of "lean" (LN(x), the qkv conv output, attn @ v, the gate product recomputed in backward) bit-identical to
    "full", on the register depthwise backward that no network test reaches, and on a padded GDFN"""
    cfg = MDTA_CASES[0]
    lnt, C, heads, B, H, W, softmax, path, seed = cfg
    x, dy, P = mdta_inputs(_mdta_tag(cfg), lnt, C, heads, B, H, W, seed)
    full, _ = mdta_hip(dev, x, dy, P, heads, mode="full")
    lean, tr = mdta_hip(dev, x, dy, P, heads, mode="lean")
    assert tr.families("dw.") == MDTA_DW["generic"], tr.counts
    _same(full, lean)
    lnt, C, hidden, B, H, W = GDFN_CASES[1]
    x, dy, P = gdfn_inputs(f"hv.gdfn-{lnt}-c{C}h{hidden}", lnt, C, hidden, B, H, W)
    full, _ = gdfn_hip(dev, x, dy, P, mode="full")
    lean, tr = gdfn_hip(dev, x, dy, P, mode="lean")
    assert tr.families("dw.") == GDFN_DW, tr.counts   # the ring backward writes the gate product on its way: no second forward
    _same(full, lean)


# ---- edge inputs --------------------------------------------------------------------------------------------------------------------
EDGE = (16, 2, 2, 6, 5)   # C, heads, B, H, W: ch = 8, ring backward
DEAD_Q, DEAD_K = (0, 3), (1, 5)   # (head, channel in the head)
DEAD_SEED = {False: 1, True: 0}


@pytest.mark.parametrize("softmax", [False, True], ids=["relu", "softmax"])
def test_mdta_dead_channels(dev, softmax):
    """an identically zero q channel (head 0) and k channel (head 1): the clamp of sq_norm_kernel, exact zeros in ghat, and in backward
    exact zeros (ReLU) or gradients of order 1 / eps (softmax: large in the reference as well, compared like everything else)"""
    C, heads, B, H, W = EDGE
    ch = C // heads
    lnt = "BiasFree" if softmax else "WithBias"
    x, dy, P = mdta_inputs(f"hv.dead{int(softmax)}", lnt, C, heads, B, H, W, DEAD_SEED[softmax])
    cq, ck = DEAD_Q[0] * ch + DEAD_Q[1], C + DEAD_K[0] * ch + DEAD_K[1]
    P["attn.qkv_dwconv.weight"][cq] = 0
    P["attn.qkv_dwconv.weight"][ck] = 0
    led, hip, t64, _ = mdta_case(dev, f"dead-{'sm' if softmax else 'relu'}", x, dy, P, heads, softmax, softmax, "ring",
                                 zero=dict(zero_rows=[DEAD_Q], zero_cols=[DEAD_K]))
    assert bool((hip["nrm"][:, [cq, ck]] == NORM_EPS).all()), hip["nrm"][:, [cq, ck]]
    assert bool((hip["ghat"][:, DEAD_Q[0], DEAD_Q[1], :] == 0).all()) and bool((hip["ghat"][:, DEAD_K[0], :, DEAD_K[1]] == 0).all())
    if not softmax:   # the dead row / column contributes exact zeros to dG, so nothing reaches the dead channel's taps
        assert bool((hip["g.attn.qkv_dwconv.weight"][[cq, ck]] == 0).all())
        assert bool((t64["g.attn.qkv_dwconv.weight"][[cq, ck]] == 0).all())
    else:
        assert float(t64["g.attn.qkv_dwconv.weight"][[cq, ck]].abs().max()) > 1e6   # order 1 / eps
    led.judge()


FAINT = 5e-13
FAINT_SEED = {False: 0, True: 0}


@pytest.mark.parametrize("softmax", [False, True], ids=["relu", "softmax"])
def test_mdta_faint_channel(dev, softmax):
    """a q channel (head 0) and a k channel (head 1) whose L2 norm over the pixels is 5e-13: below F.normalize's eps, so the forward divides
    by the clamp and the backward must NOT add the norm-path term ((n > NORM_EPS) ? ... : 0 of attn_bwd_kernel) -- with it the gradient
    of the channel would be off by about ghat^2, percent here.  (An identically zero channel cannot tell: its term is -0 either way.)"""
    C, heads, B, H, W = EDGE
    ch = C // heads
    lnt = "WithBias" if softmax else "BiasFree"
    x, dy, P = mdta_inputs(f"hv.faint{int(softmax)}", lnt, C, heads, B, H, W, FAINT_SEED[softmax])
    cq, ck = DEAD_Q[0] * ch + DEAD_Q[1], C + DEAD_K[0] * ch + DEAD_K[1]
    pre = mdta_ref(x, dy, P, torch.float64, softmax, softmax)["qkv"]
    for c in (cq, ck):   # every image's norm of the channel at or below FAINT
        P["attn.qkv_dwconv.weight"][c] *= FAINT / float(pre[:, c].flatten(1).norm(dim=1).max())
    led, hip, t64, _ = mdta_case(dev, f"faint-{'sm' if softmax else 'relu'}", x, dy, P, heads, softmax, softmax, "ring")
    n64 = t64["qkv"][:, [cq, ck]].flatten(2).norm(dim=2)
    assert float(n64.max()) <= 1.0001 * FAINT and float(n64.min()) > 0.1 * FAINT, n64
    assert bool((hip["nrm"][:, [cq, ck]] == NORM_EPS).all()), hip["nrm"][:, [cq, ck]]
    # the faint rows of ghat are no longer small against the others (|qn| = n / eps ~ 0.5), so the guard's term would be ~ ghat^2 of the gradient
    assert float(t64["ghat"][:, DEAD_Q[0], DEAD_Q[1]].abs().max()) > 0.02 and float(t64["ghat"][:, DEAD_K[0], :, DEAD_K[1]].abs().max()) > 0.02
    led.judge()


ZV_PIXELS = ((0, 1, 2, 0.0), (0, 4, 0, 0.7), (1, 5, 4, -3.0))   # (image, row, column, value of every channel)
ZV_SEED = {("WithBias", False): 0, ("BiasFree", False): 0, ("WithBias", True): 0, ("BiasFree", True): 0}


def _flatten_pixels(x):
    for b, i, j, v in ZV_PIXELS:
        x[b, :, i, j] = v
    return x


@pytest.mark.parametrize("eps_1e5", [False, True], ids=["eps1e-6", "eps1e-5"])
@pytest.mark.parametrize("lnt", ["WithBias", "BiasFree"])
def test_mdta_zero_variance_pixels(dev, lnt, eps_1e5):
    """three pixels whose channels are all equal (0, 0.7, -3.0): rstd = 1 / sqrt(eps) there, the largest gain the LayerNorm backward
    applies (and BiasFree does not centre the numerator: xn = x rstd w).  The ReLU form with eps 1e-6, the softmax form with eps 1e-5."""
    C, heads, B, H, W = EDGE
    x, dy, P = mdta_inputs(f"hv.zv{lnt}{int(eps_1e5)}", lnt, C, heads, B, H, W, ZV_SEED[lnt, eps_1e5])
    _flatten_pixels(x)
    led, hip, t64, _ = mdta_case(dev, f"zv-mdta-{lnt}-{int(eps_1e5)}", x, dy, P, heads, eps_1e5, eps_1e5, "ring")
    for b, i, j, _ in ZV_PIXELS:
        assert float(t64["rstd"][b, i * W + j]) == pytest.approx(1e5 ** 0.5 if eps_1e5 else 1e3, rel=1e-12)
    led.judge()


@pytest.mark.parametrize("eps_1e5", [False, True], ids=["eps1e-6", "eps1e-5"])
@pytest.mark.parametrize("lnt", ["WithBias", "BiasFree"])
def test_gdfn_zero_variance_pixels(dev, lnt, eps_1e5):
    C, _, B, H, W = EDGE
    x, dy, P = gdfn_inputs(f"hv.zvg{lnt}{int(eps_1e5)}", lnt, C, int(C * 2.66), B, H, W)
    _flatten_pixels(x)
    led, hip, t64, _ = gdfn_case(dev, f"zv-gdfn-{lnt}-{int(eps_1e5)}", x, dy, P, eps_1e5)
    for b, i, j, _ in ZV_PIXELS:
        assert float(t64["rstd"][b, i * W + j]) == pytest.approx(1e5 ** 0.5 if eps_1e5 else 1e3, rel=1e-12)
    led.judge()


TEMP_SEED = 0


def test_mdta_temperature_relu(dev):
    """per-head temperature (1.3, -0.7, 0.0, 2.0) under ReLU.  The head with t = 0 has attn == 0 exactly and exact zeros in everything that
    passes only through it, d temperature included (torch's ReLU gradient at 0 is 0).  The head with t = -0.7 is NOT dead: relu(t ghat) is
    positive wherever ghat is negative, in the reference as in the kernel; it is compared like the other heads, and its mask is
    asserted to be the complement of a positive head's rule (attn > 0 exactly where the reference's ghat < 0)."""
    C, heads, B, H, W = 16, 4, 2, 6, 5
    ch = C // heads
    x, dy, P = mdta_inputs("hv.temp", "BiasFree", C, heads, B, H, W, TEMP_SEED)
    P["attn.temperature"] = torch.tensor([1.3, -0.7, 0.0, 2.0]).reshape(heads, 1, 1)
    led, hip, t64, _ = mdta_case(dev, "temp-relu", x, dy, P, heads, False, False, "ring", zero=dict(zero_heads=[2]))
    off = list(range(2 * ch, 3 * ch))
    assert bool((hip["attn"][:, 2] == 0).all()) and bool((hip["out_att"][:, off] == 0).all())
    assert torch.equal(hip["attn"][:, 1] > 0, t64["ghat"][:, 1] < 0) and torch.equal(hip["attn"][:, 3] > 0, t64["ghat"][:, 3] > 0)
    rows = [p * C + c for p in range(3) for c in off]   # the q, k and v channels of the head
    for k in ("g.attn.qkv_dwconv.weight", "g.attn.qkv.weight"):
        assert bool((hip[k][rows] == 0).all()) and bool((t64[k][rows] == 0).all()), k
    assert bool((hip["g.attn.project_out.weight"][:, off] == 0).all())
    assert float(t64["g.attn.temperature"][2]) == 0 and float(hip["g.attn.temperature"][2]) == 0
    assert float(t64["g.attn.temperature"][[0, 1, 3]].abs().min()) > 0
    led.judge()


def test_mdta_temperature_softmax(dev):
    """a sharp (t = 30) and a flat (t = 0.01) softmax head: every row of attn sums to 1 within 4 ulp"""
    C, heads, B, H, W = EDGE
    x, dy, P = mdta_inputs("hv.tempsm", "WithBias", C, heads, B, H, W)
    P["attn.temperature"] = torch.tensor([30.0, 0.01]).reshape(heads, 1, 1)
    led, hip, t64, _ = mdta_case(dev, "temp-sm", x, dy, P, heads, True, True, "ring")
    assert float((hip["attn"].double().sum(-1) - 1).abs().max()) <= 4 * 2.0 ** -23
    assert float(t64["attn"][:, 0].max()) > 0.5 and float(t64["attn"][:, 1].max()) < 0.2   # sharp and flat in the reference
    led.judge()


GELU_SCALE = 2.0


def test_gdfn_gelu_tails(dev):
    """project_in scaled so that the float64 x1 spans at least [-6, 6]: the exact-erf GELU where gelu(x) is x or ~ -0 and gelu' 1 or 0"""
    x, dy, P = gdfn_inputs("hv.tails", "WithBias", 16, int(16 * 2.66), 1, 7, 9)
    P["ffn.project_in.weight"] *= GELU_SCALE
    led, hip, t64, _ = gdfn_case(dev, "gelu-tails", x, dy, P)
    assert float(t64["x1"].min()) <= -6 and float(t64["x1"].max()) >= 6, (float(t64["x1"].min()), float(t64["x1"].max()))
    led.judge()
