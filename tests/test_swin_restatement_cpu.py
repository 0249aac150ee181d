"""CPU: the float64 restatement of the SwinIR halves (tests/swin_restatement.py) against an independent composition of torch's own ops and
against the golden vectors of the real reference, and the sensitivity of every case of tests/test_gpu_swin_halves.py: a restatement with
one deliberate mistake (swin_restatement.MUTATIONS) must leave the right one by at least 10 x the bound the GPU test holds a tensor to, on at
least one tensor that test compares -- a case that could not tell the mistake from the kernel would test nothing.

The case tables, the input builders, the error measure and K of the GPU test live here, so that both files see the same tensors and the
same bound.  Seeds, ranges and scales are chosen so that every condition the GPU test states about its inputs (saturation range, GELU span,
zero-variance pixels) holds for the float64 reference alone; they are asserted below.

MUTATION TABLE (EXPECT): per mutation, a rule over the runs -- True: the run must detect it, False: it cannot (the reason is with the
rule), None: left open (it may, by a margin that is not reasoned here).  Every mutation has at least one run that must detect it, and the
whole table is asserted, so an edit of the case list cannot silently drop a detector.  Where a rule is narrower than "every case with shift
> 0" the reason is geometry, not tolerance:
  * roll sign flipped (consistently, on the way in and out): the windows are the same SETS of pixels wherever an axis is one window
    wide (the whole axis wraps: any shift gives the same set) or 2 shift = 0 mod ws, and attention without position bias does not see
    the order inside a window.  So the 2 x 2 map with ws = 2 cannot tell it, every other shifted case can.
  * shift on one axis only: two mutants, one per axis that keeps its shift.  A case whose OTHER axis is one window wide cannot tell
    (H == ws loses nothing when the y shift is dropped).  Every shifted case with a second window on some axis detects one of the two;
    the 2 x 2 map detects neither.
  * (i, j) transposed inside the window and the window grid transposed are mistakes only where the way in and the way out disagree (a
    consistent relabelling of tokens or windows computes the same thing): (i, j) is transposed on the way out only; the grid mutant
    divides the window number by nwy instead of nwx, which is the identity where nwy == nwx and leaves the map where they differ.
  * qkv columns as (heads, 3, hd) is the right layout when heads == 1.
  * pad head channels leaking into the next head needs a next head and pad channels.
  * lse without the max shows only where exp overflows fp32, i.e. in the saturated runs (it is evaluated in fp32: float64 carries e^200).
  * eps 1e-6 moves rstd by 4e-6 of itself at the variance of these inputs, within 10 x the bound; a zero-variance pixel has
    rstd = 1000 instead of 316."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import swin_restatement as R
from dcpt_amd.keyed_init import keyed_input, keyed_tensor

K = 10                           # twice the worst measured HIP / oracle32 ratio (4.90), rounded up: see tests/test_gpu_swin_halves.py
CAPS = (5e-5, 2e-4, 3e-4)        # tests/test_gpu_swinir.py: y / dx / parameter gradients, whole-tensor number
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- cases ---------------------------------------------------------------------------------------------------------------------------
#              C   heads ws shift B  H   W
ATTN_CASES = [(12, 4, 1, 0, 2, 3, 5),        # N = 1, hd = 3
              (8, 2, 2, 1, 3, 2, 2),         # N = 4, one window per image: both axes wrap entirely
              (36, 1, 3, 2, 1, 6, 9),        # N = 9 (odd kn), hd = 36: DP 64 with NP 32, shift ws - 1, nwy != nwx
              (132, 4, 5, 3, 1, 5, 10),      # N = 25, hd = 33 (odd kd in the 64-column form), H == ws with a shift
              (96, 2, 6, 5, 1, 12, 6),       # N = 36: NP 64, hd = 48, all four S tiles and four O tiles partly padded, nwx = 1
              (56, 2, 7, 3, 2, 7, 14),       # N = 49, hd = 28: NP 64 with DP 32 (two O tiles)
              (180, 6, 8, 1, 1, 8, 16),      # default width, shift 1
              (64, 1, 8, 7, 1, 16, 8)]       # hd = 64 exact, shift 7
#             C   hidden B  H  W
MLP_CASES = [(4, 8, 1, 1, 1),                # M = 1
             (12, 24, 2, 3, 5),
             (20, 52, 1, 7, 9),              # hidden is no multiple of C
             (16, 64, 2, 4, 3),
             (180, 360, 1, 4, 6)]
WS7, WS3 = ATTN_CASES[5], ATTN_CASES[2]
SAT_SCALE = {7: 6.2, 3: 6.0}    # on qkv.weight: the scaled scores of the float64 reference spread past +-60, max|lse| in [60, 200]
ZV_ATTN = (WS7, ((0, 1, 2, 0.0), (0, 4, 0, 0.7), (1, 5, 4, -3.0)))        # (image, row, column, value of every channel)
ZV_MLP = (MLP_CASES[1], ((0, 1, 2, 0.0), (0, 2, 0, 0.7), (1, 0, 4, -3.0)))
TAILS_CASE, TAILS_SCALE = MLP_CASES[2], 3.0       # on fc1.weight: h of the float64 reference spans at least [-8, 8]
#        run id: (half, case, variant)
RUNS = {**{"a-" + "-".join(map(str, c)): ("attn", c, "plain") for c in ATTN_CASES},
        "sat-ws7": ("attn", WS7, "sat"), "sat-ws3": ("attn", WS3, "sat"), "zv-attn": ("attn", WS7, "zv"),
        **{"m-" + "-".join(map(str, c)): ("mlp", c, "plain") for c in MLP_CASES},
        "zv-mlp": ("mlp", ZV_MLP[0], "zv"), "gelu-tails": ("mlp", TAILS_CASE, "tails")}
ATTN_RUNS = [r for r, v in RUNS.items() if v[0] == "attn"]
MLP_RUNS = [r for r, v in RUNS.items() if v[0] == "mlp"]
ATTN_KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias")
MLP_KEYS = ("norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def block_shapes(C, hidden):
    return {"norm1.weight": (C,), "norm1.bias": (C,), "attn.qkv.weight": (3 * C, C), "attn.qkv.bias": (3 * C,), "attn.proj.weight": (C, C),
            "attn.proj.bias": (C,), "norm2.weight": (C,), "norm2.bias": (C,), "mlp.fc1.weight": (hidden, C), "mlp.fc1.bias": (hidden,),
            "mlp.fc2.weight": (C, hidden), "mlp.fc2.bias": (C,)}


@functools.lru_cache(maxsize=None)
def inputs(run):
    """-> x, dy (B, C, H, W), P: fp32 CPU tensors.  x has a per-channel offset, so mu is a stage worth looking at"""
    half, case, variant = RUNS[run]
    C, B, H, W = (case[0], *case[-3:])
    tag = "swh." + run
    x = keyed_input(tag + ".x", (B, C, H, W), lo=-2.0, hi=2.0) + keyed_input(tag + ".xo", (1, C, 1, 1), lo=-1.0, hi=1.0)
    dy = keyed_input(tag + ".dy", (B, C, H, W), lo=-1.0, hi=1.0)
    shapes = block_shapes(C, case[1] if half == "mlp" else 2 * C)
    P = {k: keyed_tensor(f"{tag}.{k}", shapes[k]) for k in (ATTN_KEYS if half == "attn" else MLP_KEYS)}
    if variant == "sat":
        P["attn.qkv.weight"] *= SAT_SCALE[case[2]]
    if variant == "tails":
        P["mlp.fc1.weight"] *= TAILS_SCALE
    if variant == "zv":
        for b, i, j, v in (ZV_ATTN if half == "attn" else ZV_MLP)[1]:
            x[b, :, i, j] = v
    return x, dy, P


def reference(run, dtype, mut=()):
    half, case, _ = RUNS[run]
    x, dy, P = inputs(run)
    if half == "attn":
        return R.attn_grads(x, dy, P, *case[1:4], dtype, mut)
    return R.mlp_grads(x, dy, P, dtype, mut)


@functools.lru_cache(maxsize=None)
def refs(run):
    """(float64 truth, float32 yardstick) of a run: computed once, shared by every test of both files, never written to"""
    return reference(run, torch.float64), reference(run, torch.float32)


# ---- the error measure (tests/test_gpu_restormer_halves.py) -----------------------------------------------------------------------------
def per_image(B):
    return lambda v: v.reshape(B, -1)


def per_row(v):             # output row of a weight; entry of a bias / norm vector
    return v.reshape(v.shape[0], -1)


def per_head(v):            # lse (M, heads)
    return v.t()


def per_block(n):           # qkv (M, 3C): 3 heads blocks of hd columns; att (M, C): heads blocks
    return lambda v: v.reshape(v.shape[0], n, -1).permute(1, 0, 2).reshape(n, -1)


def _ulp_rel(m, of=None):
    """one fp32 ulp of the magnitude ``of`` (default: m itself) relative to m"""
    m, of = float(m), float(m if of is None else of)
    return float(np.spacing(np.float32(of))) / m if m > 0 else 0.0


def numbers(a, t, sl, mag=None):
    """(whole, floor of whole, worst slice, floor of that slice), all relative to the largest magnitude of the truth.  ``mag``: per slice,
    the magnitude the floor's ulp is taken of where that is not the slice's own largest value (the terms of a sum)"""
    a2, t2 = sl(a.double()), sl(t.double())
    assert a2.shape == t2.shape, (a2.shape, t2.shape)
    d = (a2 - t2).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    dm, tm = d.amax(1), t2.abs().amax(1)
    mag = tm if mag is None else mag.double().flatten()
    assert mag.shape == tm.shape and bool((mag >= tm).all())
    e = torch.where(tm > 0, dm / tm.clamp_min(1e-300), torch.where(dm == 0, torch.zeros_like(dm), torch.full_like(dm, math.inf)))
    i = int(e.argmax())
    wm = float(tm.max())
    whole = float(dm.max()) / wm if wm > 0 else (0.0 if float(dm.max()) == 0 else math.inf)
    return whole, _ulp_rel(wm, mag.max()), float(e[i]), _ulp_rel(tm[i], mag[i])


def compared(run):
    """[(name, pick, slicer, cap, mag key or None, lse floor?)] of a run: what the GPU test compares and how.  ``pick`` cuts the part of
    the tensor that is compared (the key part of qkv.bias is judged on its own: its truth is zero in exact arithmetic)"""
    half, case, _ = RUNS[run]
    C, B = case[0], case[-3]
    whole = slice(None)
    out = [("mu", whole, per_image(B), None, None, False), ("rstd", whole, per_image(B), None, None, False)]
    if half == "attn":
        heads = case[1]
        out += [("qkv", whole, per_block(3 * heads), None, None, False), ("lse", whole, per_head, None, None, False),
                ("att", whole, per_block(heads), None, None, False)]
        keys = ATTN_KEYS
    else:
        out += [("h", whole, per_image(B), None, None, False)]
        keys = MLP_KEYS
    out += [("y", whole, per_image(B), CAPS[0], None, False), ("dx", whole, per_image(B), CAPS[1], None, True)]
    for k in keys:
        summed = k.endswith(".bias") or k.startswith("norm")
        if k in ("attn.qkv.bias", "attn.qkv.weight") and case[2] == 1:
            # N = 1: P = 1 whatever the score, so the q and k parts are zero in exact arithmetic as well (test_single_token_window)
            out.append(("g." + k + "[v]", slice(2 * C, 3 * C), per_row, CAPS[2], "mag.g." + k if summed else None, True))
        elif k == "attn.qkv.bias":
            out += [("g." + k + "[q]", slice(0, C), per_row, CAPS[2], "mag.g." + k, True),
                    ("g." + k + "[v]", slice(2 * C, 3 * C), per_row, CAPS[2], "mag.g." + k, True)]
        else:
            out.append(("g." + k, whole, per_row, CAPS[2], "mag.g." + k if summed else None, True))
    return out


def lse_term(run, t64):
    """what the floors of dx and the gradients gain in a saturated run: the backward's P = exp(S - lse) inherits the rounding of the fp32
    lse, a relative error of up to 2^-24 |lse| that plain softmax autograd (the float32 yardstick) does not have"""
    return 2.0 ** -24 * float(t64["lse"].abs().max()) if RUNS[run][2] == "sat" else 0.0


def judged(run, got, t64, o32):
    """[(name, (whole, slice) of ``got``, (whole, slice) of the float32 oracle, the two floors, cap)] over everything compared(run) lists"""
    out = []
    for name, pick, sl, cap, mk, lsef in compared(run):
        key = name.split("[")[0]
        mag = t64[mk][pick] if mk else None
        wa, fw, sa, fs = numbers(got[key][pick], t64[key][pick], sl, mag)
        wo, _, so, _ = numbers(o32[key][pick], t64[key][pick], sl, mag)
        extra = lse_term(run, t64) if lsef else 0.0
        out.append((name, (wa, sa), (wo, so), (fw + extra, fs + extra), cap))
    return out


# ---- the independent composition --------------------------------------------------------------------------------------------------------
def torch_attn(x, P, heads, ws, shift):
    B, C, H, W = x.shape
    hd, N = C // heads, ws * ws
    t = x.permute(0, 2, 3, 1)
    xn = F.layer_norm(t, (C,), P["norm1.weight"], P["norm1.bias"], 1e-5)
    qkv_map = F.linear(xn, P["attn.qkv.weight"], P["attn.qkv.bias"])
    h = torch.roll(xn, (-shift, -shift), (1, 2))
    win = h.reshape(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, C)
    qkv = F.linear(win, P["attn.qkv.weight"], P["attn.qkv.bias"]).reshape(-1, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = (qkv[0] * hd ** -0.5) @ qkv[1].transpose(-2, -1)

    def back(w):     # (nw, N, cols) -> (M, cols) in pixel order
        w = w.reshape(B, H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)
        return torch.roll(w, (shift, shift), (1, 2)).reshape(B * H * W, -1)

    att = back((torch.softmax(s, -1) @ qkv[2]).transpose(1, 2).reshape(-1, N, C))
    lse = back(torch.logsumexp(s, -1).transpose(1, 2))
    y = t.reshape(-1, C) + F.linear(att, P["attn.proj.weight"], P["attn.proj.bias"])
    return dict(mu=t.mean(-1).flatten(), rstd=1.0 / torch.sqrt(t.var(-1, unbiased=False).flatten() + 1e-5), xn=xn.reshape(-1, C),
                qkv=qkv_map.reshape(-1, 3 * C), lse=lse, att=att, y=y.reshape(B, H, W, C).permute(0, 3, 1, 2))


def torch_mlp(x, P):
    B, C, H, W = x.shape
    t = x.permute(0, 2, 3, 1)
    xn = F.layer_norm(t, (C,), P["norm2.weight"], P["norm2.bias"], 1e-5)
    h = F.linear(xn, P["mlp.fc1.weight"], P["mlp.fc1.bias"])
    y = t + F.linear(F.gelu(h), P["mlp.fc2.weight"], P["mlp.fc2.bias"])
    return dict(mu=t.mean(-1).flatten(), rstd=1.0 / torch.sqrt(t.var(-1, unbiased=False).flatten() + 1e-5), xn=xn.reshape(-1, C),
                h=h.reshape(-1, h.shape[-1]), y=y.permute(0, 3, 1, 2))


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("run", list(RUNS))
def test_restatement_equals_torch_composition(run):
    half, case, _ = RUNS[run]
    x, dy, P = inputs(run)
    t64 = refs(run)[0]
    Pd = {k: v.double().requires_grad_(True) for k, v in P.items()}
    xd = x.double().requires_grad_(True)
    st = torch_attn(xd, Pd, *case[1:4]) if half == "attn" else torch_mlp(xd, Pd)
    st["y"].backward(dy.double())
    for k, v in st.items():
        assert rel(t64[k], v) <= 1e-12, (k, rel(t64[k], v))
    assert rel(t64["dx"], xd.grad) <= 1e-12
    for k, p in Pd.items():
        g, m = t64["g." + k], t64.get("mag.g." + k)
        if m is None:
            assert rel(g, p.grad) <= 1e-12, k
        else:   # a sum over the tokens: two float64 evaluations agree to 1e-12 of what was summed (the key part of qkv.bias sums to ~0)
            assert bool(((g - p.grad).abs() <= 1e-12 * m).all()) and bool((m * (1 + 1e-12) >= g.abs()).all()), k


# ---- the golden vectors of the real reference ---------------------------------------------------------------------------------------
BLOCKS = [("c180_s0", 180, 6, 8, 0, 1, 8, 24), ("c180_s4", 180, 6, 8, 4, 1, 8, 24),
          ("c60_ws4_s0", 60, 6, 4, 0, 2, 12, 16), ("c60_ws4_s2", 60, 6, 4, 2, 2, 12, 16)]
SUB = 29   # tools/make_golden_swinir.py: large gradients are stored as every 29th element


@pytest.mark.parametrize("tag,C,heads,ws,shift,B,H,W", BLOCKS)
def test_halves_compose_to_the_golden_block(tag, C, heads, ws, shift, B, H, W):
    """attn_half then mlp_half with the keyed weights and inputs of test_block_golden (tests/test_gpu_swinir.py) reproduce the real
    reference's y, dx and gradients within that test's tolerances"""
    g = np.load(os.path.join(GOLDEN, f"swinir_block_{tag}.npz"))
    P = {k: keyed_tensor(f"swb_{tag}." + k, s).double().requires_grad_(True) for k, s in block_shapes(C, 2 * C).items()}
    x = keyed_input(f"swb_{tag}.x", (B, C, H, W), lo=-1.0, hi=1.0).double().requires_grad_(True)
    go = keyed_input(f"swb_{tag}.go", (B, C, H, W), lo=-1.0, hi=1.0).double()
    y = R.mlp_half(R.attn_half(x, P, heads, ws, shift)["y"], P)["y"]
    y.backward(go)
    assert rel(y, torch.from_numpy(g["y"])) <= 5e-5 and rel(x.grad, torch.from_numpy(g["dx"])) <= 2e-4
    for k, p in P.items():
        if "g." + k in g:
            assert rel(p.grad, torch.from_numpy(g["g." + k])) <= 3e-4, k
        else:
            assert rel(p.grad.flatten()[::SUB], torch.from_numpy(g["gsub." + k])) <= 3e-4, k


# ---- the conditions the GPU test states about its inputs --------------------------------------------------------------------------
def scaled_scores(run):
    """(nw, heads, N, N) of the float64 reference, from its qkv stage"""
    _, (C, heads, ws, shift, B, H, W), _ = RUNS[run]
    qkv = refs(run)[0]["qkv"]
    hd = C // heads
    q, k, _ = qkv[R.window_rows(B, H, W, ws, shift, shift)].reshape(-1, ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
    return (q * hd ** -0.5) @ k.transpose(-1, -2)


@pytest.mark.parametrize("run", ["sat-ws7", "sat-ws3"])
def test_saturated_inputs(run):
    s = scaled_scores(run)
    lse = float(refs(run)[0]["lse"].abs().max())
    pmax = torch.softmax(s, -1).amax(-1)
    share = float((pmax > 1 - 2.0 ** -24).double().mean())
    print(f"{run}: scores {float(s.min()):.1f} .. {float(s.max()):.1f}, max|lse| {lse:.1f}, rows with p_max > 1 - 2^-24: {share:.2f}")
    assert float(s.min()) <= -60 and float(s.max()) >= 60 and 60 <= lse <= 200 and share >= 0.25


def test_plain_attention_inputs_are_benign():
    """the unsaturated runs stay where fp32 lse costs nothing: max|lse| < 16, so 2^-24 |lse| is below an ulp of P"""
    for run in ATTN_RUNS:
        if RUNS[run][2] != "sat":
            assert float(refs(run)[0]["lse"].abs().max()) < 16, run


def test_gelu_tail_inputs():
    h = refs("gelu-tails")[0]["h"]
    print(f"gelu-tails: h {float(h.min()):.2f} .. {float(h.max()):.2f}")
    assert float(h.min()) <= -8 and float(h.max()) >= 8


@pytest.mark.parametrize("run", ["zv-attn", "zv-mlp"])
def test_zero_variance_inputs(run):
    half, case, _ = RUNS[run]
    H, W = case[-2:]
    t64 = refs(run)[0]
    for b, i, j, v in (ZV_ATTN if half == "attn" else ZV_MLP)[1]:
        m = (b * H + i) * W + j
        assert float(t64["rstd"][m]) == pytest.approx(1e5 ** 0.5, rel=1e-12) and float(t64["mu"][m]) == pytest.approx(float(np.float32(v)), abs=1e-15)


def cancelled_magnitude(run):
    """(C,) the magnitude of what cancels in d qkv.bias[C:2C] when dS = P (dP - D) is formed in fp32:  d k-bias[c] = sum_i (sum_m dS[i, m])
    scale q[i, c], and the inner sum is zero only up to the rounding of its terms P dP and P D -- sum_i sum_m P[i, m] (|dP[i, m]| + |D[i]|)
    scale |q[i, c]|.  Where the rows are one-hot dS itself is all but cancelled (dP - D ~ 0 at the hot key) and this is far above the sum of
    |dk| rows; elsewhere it is a small multiple of it."""
    _, (C, heads, ws, shift, B, H, W), _ = RUNS[run]
    x, dy, P = inputs(run)
    hd, N = C // heads, ws * ws
    idx = R.window_rows(B, H, W, ws, shift, shift)
    q, k, v = refs(run)[0]["qkv"][idx].reshape(-1, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    p = torch.softmax((q * hd ** -0.5) @ k.transpose(-1, -2), -1)
    dO = (dy.double().permute(0, 2, 3, 1).reshape(-1, C) @ P["attn.proj.weight"].double())[idx].reshape(-1, N, heads, hd).permute(0, 2, 1, 3)
    dP = dO @ v.transpose(-1, -2)
    D = (p * dP).sum(-1, keepdim=True)
    per_query = (p * (dP.abs() + D.abs())).sum(-1, keepdim=True)           # (nw, heads, N, 1)
    return (per_query * q.abs() * hd ** -0.5).sum((0, 2)).reshape(C)


def key_bias_floor(run):
    """one fp32 ulp of the sum of magnitudes of the rows d qkv.bias[C:2C] column-sums; in the saturated runs of cancelled_magnitude"""
    C = RUNS[run][1][0]
    m = cancelled_magnitude(run) if RUNS[run][2] == "sat" else refs(run)[0]["mag.g.attn.qkv.bias"][C:2 * C]
    return torch.from_numpy(np.spacing(m.float().numpy())).double()


def test_key_bias_gradient_is_zero_in_exact_arithmetic():
    """adding a constant vector to every key moves each score row by a constant: float64 leaves 1e-13 of what it summed at the most, and
    the float32 oracle stays within the floor the GPU test applies"""
    for run in ATTN_RUNS:
        C = RUNS[run][1][0]
        t64, o32 = refs(run)
        g, m = t64["g.attn.qkv.bias"][C:2 * C], t64["mag.g.attn.qkv.bias"][C:2 * C]
        assert bool((g.abs() <= 1e-13 * m).all()), (run, float((g.abs() / m.clamp_min(1e-300)).max()))
        if RUNS[run][1][2] > 1:
            m2 = cancelled_magnitude(run)
            assert float(m.min()) > 0 and bool((m2 >= m).all()), run
            assert bool((o32["g.attn.qkv.bias"][C:2 * C].double().abs() <= K * key_bias_floor(run)).all()), run
            print(f"{run}: cancelled magnitude / sum|dk rows| {float((m2 / m).min()):.1f} .. {float((m2 / m).max()):.1f}")


# ---- the mutation table ------------------------------------------------------------------------------------------------------------------
def _geo(run):
    half, case, variant = RUNS[run]
    if half != "attn":
        return None
    C, heads, ws, shift, B, H, W = case
    return dict(C=C, heads=heads, ws=ws, shift=shift, hd=C // heads, N=ws * ws, nwy=H // ws, nwx=W // ws, variant=variant)


def _attn(rule):
    """a rule over the attention runs; MLP runs do not run an attention mutant"""
    return lambda run: rule(_geo(run)) if _geo(run) else "skip"


def _sets_differ(g):   # the windows with the shift negated are other sets of pixels on some axis
    return g["shift"] > 0 and any(n > 1 and (2 * g["shift"]) % g["ws"] != 0 for n in (g["nwy"], g["nwx"]))


EXPECT = {
    "roll_sign": _attn(_sets_differ),
    "no_inverse_roll": _attn(lambda g: g["shift"] > 0),
    "shift_y_only": _attn(lambda g: g["shift"] > 0 and g["nwx"] > 1),       # the x shift is dropped
    "shift_x_only": _attn(lambda g: g["shift"] > 0 and g["nwy"] > 1),       # the y shift is dropped
    "clamp": _attn(lambda g: g["shift"] > 0),
    "ij_transposed": _attn(lambda g: g["ws"] > 1),
    "grid_transposed": _attn(lambda g: g["nwy"] != g["nwx"]),
    "qkv_heads_first": _attn(lambda g: g["heads"] > 1),
    "scale_dp": _attn(lambda g: g["hd"] not in (32, 64)),
    # (a saturated row whose largest score is far above 0 does not see pad keys of score 0: e^(0 - max) is nothing)
    "pad_keys": _attn(lambda g: g["N"] not in (32, 64) and (None if g["variant"] == "sat" else True)),
    "v_pad_leak": _attn(lambda g: g["heads"] > 1 and g["hd"] not in (32, 64)),
    "lse_no_max": _attn(lambda g: g["variant"] == "sat"),
    "lse_unscaled": _attn(lambda g: True),
    "eps_1e6": lambda run: True if RUNS[run][2] == "zv" else None,
    "unbiased_var": lambda run: True,                                       # 1 / 2C of rstd: 0.3 % at C = 180
    "tanh_gelu": lambda run: "skip" if _geo(run) else (True if run == "gelu-tails" or RUNS[run][1][:2] == (180, 360) else None),
    "gelu_no_xpdf": lambda run: "skip" if _geo(run) else True,
}


def detects(run, mut):
    """the compared tensors on which the mutant leaves the float64 restatement by >= 10 x the bound the GPU test applies there"""
    t64, o32 = refs(run)
    got = reference(run, torch.float64, (mut,))
    hit = []
    for name, (wa, sa), (wo, so), (fw, fs), cap in judged(run, got, t64, o32):
        if (wa > 0 and wa >= 10 * (K * wo + fw)) or (sa > 0 and sa >= 10 * (K * so + fs)):
            hit.append(name)
    return hit


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutation_table(mut):
    assert set(EXPECT) == set(R.MUTATIONS)
    want = {run: EXPECT[mut](run) for run in RUNS}
    assert any(w is True for w in want.values()), f"{mut}: no run must detect it"
    got = {run: detects(run, mut) for run, w in want.items() if w != "skip"}
    print(f"{mut}: " + ", ".join(f"{r}{'*' if want[r] is None else ''} {len(h)}" for r, h in got.items()) + "   (tensors moved; * = left open)")
    wrong = {r: h for r, h in got.items() if want[r] is not None and bool(h) != want[r]}
    assert not wrong, f"{mut}: expected {({r: want[r] for r in wrong})}, moved {wrong}"


def test_shifted_cases_detect_a_one_axis_shift():
    """every shifted case with a second window on some axis tells at least one of the two one-axis mutants"""
    for run in ATTN_RUNS:
        g = _geo(run)
        if g["shift"] > 0 and (g["nwy"] > 1 or g["nwx"] > 1):
            assert EXPECT["shift_y_only"](run) or EXPECT["shift_x_only"](run), run
