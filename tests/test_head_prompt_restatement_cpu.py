"""CPU: the float64 restatements of tests/head_prompt_restatement.py against torch's own float64 ops, and the sensitivity of every case of
tests/test_gpu_head_prompt_ops.py: a restatement with one deliberate index / routing mistake must move at least one output of the case
by 10x the tolerance the GPU test holds that output to -- a case that could not tell the mistake from the kernel would test nothing.

The case tables and the input builders of the GPU test live here, so that both files see the same tensors."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_prompt_restatement as R
from dcpt_amd.keyed_init import keyed_input, keyed_tensor

# scale-relative max-error tolerances of the GPU test (those of test_promptgen_golden, test_mix_and_head, test_conv_pool_relu and
# test_dc_img_head_golden)
TOL = {
    "prompt": {"y": 1e-5, "dlogits": 1e-4, "dparam": 1e-4},
    "meanpool": {"logits": 1e-5, "dx": 1e-5, "dfw": 1e-5, "dfb": 1e-5},
    "pool": {"y": 1e-5, "dx": 1e-4, "dw": 1e-4},
    "mix": {"y": 1e-6, "dfeat": 1e-6, "dprev": 1e-7, "dmix": 1e-5},
    "embed": {"y": 2e-5, "dx": 1e-4, "dw": 1e-4, "db": 1e-4, "dlnw": 1e-4, "dlnb": 1e-4},
}

# ---- cases ---------------------------------------------------------------------------------------------------------------------
# (B, L, D, S, H, W, amp): logits uniform in +-amp
PROMPT_CASES = [
    (3, 5, 8, 6, 13, 9, 2), (3, 5, 8, 6, 4, 5, 2), (3, 5, 8, 6, 6, 6, 2),   # the geometries of test_promptgen_golden
    (2, 5, 4, 1, 7, 5, 2),            # S = 1
    (2, 5, 4, 2, 9, 3, 2),            # S = 2
    (1, 1, 8, 5, 1, 11, 2),           # L = 1, H = 1
    (2, 8, 8, 4, 10, 1, 2),           # L = MAXL, W = 1
    (2, 5, 12, 16, 3, 5, 2),          # 5.33x / 3.2x down: source pixels outside every footprint; D % 8 != 0
    (1, 5, 8, 3, 50, 7, 2),           # 16.7x up in H
    (2, 5, 8, 7, 5, 23, 2),           # down in H, up in W
    (65, 5, 4, 4, 6, 6, 2),           # the softmax kernel's second block
    (1, 5, 64, 64, 64, 64, 2), (1, 5, 128, 32, 40, 24, 2), (1, 5, 320, 16, 20, 17, 2),   # the network's prompts, on / off their size
    (1, 5, 64, 8, 520, 512, 2),       # 4.26 M quads > 16384 x 256: a thread's second element
    (3, 5, 8, 6, 13, 9, 80),          # softmax stability
    (2, 5, 8, 4, 7, 9, 100),          # ... past log(FLT_MAX) = 88.7: exp(logit) itself overflows fp32 (e^80 does not)
]
# (B, C, H, W, NC), P = H * W
MEANPOOL_CASES = [(1, 4, 1, 1, 1), (3, 12, 7, 9, 5), (2, 40, 8, 8, 7), (2, 64, 1, 127, 10), (2, 64, 8, 16, 10), (3, 12, 10, 13, 5),
                  (1, 40, 1, 191, 7), (2, 64, 37, 109, 10), (1, 192, 17, 241, 5), (2, 1028, 50, 82, 6)]
# (B, Cin, Cout, H, W)
POOL_RANDOM = [(1, 12, 20, 2, 6), (2, 8, 16, 6, 10), (1, 8, 32, 1024, 1032)]
POOL_SPECIAL = ["quad", "top", "left", "const", "neg", "zero"]     # at (2, 8, 16, 8, 12)
# (shape, n, idx, amp): amp None = keyed mixing weights (N(0, 0.5)), else uniform in +-amp
MIX_CASES = [((1, 4, 1, 1), 1, 0, None), ((2, 16, 6, 6), 4, 0, None), ((2, 16, 6, 6), 4, 3, None), ((1, 12, 5, 7), 64, 63, None),
             ((3, 20, 9, 11), 5, 2, 50), ((1, 4, 1450, 1450), 4, 1, None)]
EMBED_SHAPES = [(2, 3, 1, 1), (1, 3, 2, 9), (1, 3, 7, 8), (1, 3, 37, 29), (2, 3, 36, 28)]
EMBED_DIM = 8


def case_id(c):
    if not isinstance(c, tuple):
        return str(c)
    return "-".join(case_id(v).replace("-", "x") if isinstance(v, tuple) else str(v) for v in c)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def prompt_inputs(case):
    """-> logits, param, dout (dout holds bf16 values: the bf16 run gets the same numbers)"""
    B, L, D, S, H, W, amp = case
    tag = "hp.pm." + case_id(case)
    return (keyed_input(tag + ".lg", (B, L), lo=-amp, hi=amp), keyed_tensor(tag + ".pp", (1, L, D, S, S)),
            keyed_input(tag + ".do", (B, D, H, W), lo=-1, hi=1).bfloat16().float())


def meanpool_inputs(case):
    """-> x (non-zero mean: the long sums do not cancel), fw, fb, g"""
    B, C, H, W, NC = case
    tag = "hp.mp." + case_id(case)
    return (keyed_input(tag + ".x", (B, C, H, W), lo=-0.5, hi=1.5), keyed_tensor(tag + ".fc.weight", (NC, C)),
            keyed_tensor(tag + ".fc.bias", (NC,)), keyed_input(tag + ".go", (B, NC), lo=-1, hi=1))


def pool_inputs(case):
    """-> x, w, dy.  The special cases: 2 x 2 windows of four equal pixels (quad), with the top row (top) or the left column (left)
    duplicated, one pixel everywhere (const), every conv output negative (neg), a zero image (zero)."""
    B, Cin, Cout, H, W = case if isinstance(case, tuple) else (2, 8, 16, 8, 12)
    tag = "hp.pl." + case_id(case)
    x = keyed_input(tag + ".x", (B, Cin, H, W), lo=-1, hi=1)
    w = keyed_tensor(tag + ".conv.weight", (Cout, Cin, 1, 1))
    dy = keyed_input(tag + ".go", (B, Cout, H // 2, W // 2), lo=-1, hi=1)
    if case == "quad":
        x = x[..., 0::2, 0::2].repeat_interleave(2, 2).repeat_interleave(2, 3)
    elif case == "top":
        x[..., 0::2, 1::2] = x[..., 0::2, 0::2]
    elif case == "left":
        x[..., 1::2, 0::2] = x[..., 0::2, 0::2]
    elif case == "const":
        x = x[:, :, :1, :1].expand(B, Cin, H, W)
    elif case == "neg":
        x, w = x.abs() + 0.1, -(w.abs() + 0.01)
    elif case == "zero":
        x = torch.zeros_like(x)
    return x.contiguous(), w, dy


def mix_inputs(case):
    """-> prev, feat, mixing weights, dout"""
    shape, n, idx, amp = case
    tag = "hp.mx." + case_id(case)
    mw = keyed_tensor(tag + ".mixing_weights", (n,)) if amp is None else keyed_input(tag + ".mw", (n,), lo=-amp, hi=amp)
    return (keyed_input(tag + ".p", shape, lo=-1, hi=1), keyed_input(tag + ".f", shape, lo=-1, hi=1), mw,
            keyed_input(tag + ".go", shape, lo=-1, hi=1))


def embed_inputs(shape):
    """-> x, conv weight, conv bias, LayerNorm weight, LayerNorm bias, dy"""
    B, Cin, H, W = shape
    tag = "hp.em." + case_id(shape)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    return (keyed_input(tag + ".x", shape), keyed_tensor("hp.em.conv.weight", (EMBED_DIM, Cin, 7, 7)),
            keyed_tensor("hp.em.conv.bias", (EMBED_DIM,)), keyed_tensor("hp.em.norm.weight", (EMBED_DIM,)),
            keyed_tensor("hp.em.norm.bias", (EMBED_DIM,)), keyed_input(tag + ".go", (B, EMBED_DIM, Ho, Wo), lo=-1, hi=1))


def pool_slices(P):
    """the pixel slices of the mean-pool kernel (dchead.hip): -> (slices, pixels per slice)"""
    nsl = min(max(P // 64, 1), 64)
    return nsl, -(-P // nsl)


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def moved(mut, ref):
    """scale-relative distance of a mutant's output from the restatement's (infinite when the mutant is not finite)"""
    mut, ref = mut.detach().double(), ref.detach().double()
    if not bool(torch.isfinite(mut).all()):
        return float("inf")
    scale = float(ref.abs().max()) or float(mut.abs().max()) or 1.0
    return float((mut - ref).abs().max()) / scale


def detected(op, ref, mutants, lazy=False):
    """{mutant name: [outputs it moves by >= 10 x their tolerance]}; ``lazy``: stop at the first mutant that is detected"""
    out = {}
    for name, run in mutants:
        mut = run()
        out[name] = [k for k, tol in TOL[op].items() if k in mut and k in ref and moved(mut[k], ref[k]) >= 10 * tol]
        if lazy and out[name]:
            break
    return out


def swapped(attr, fn, run):
    """run() with R.<attr> replaced by fn"""
    keep = getattr(R, attr)
    setattr(R, attr, fn)
    try:
        return run()
    finally:
        setattr(R, attr, keep)


# ---- prompt mix ----------------------------------------------------------------------------------------------------------------
def lerp_variant(S, n_dst, fused=False, half=True, clamp_src=True, clamp_i1=True):
    """R.lerp_matrix with a switch per mistake; a neighbour outside 0 .. S-1 contributes nothing"""
    dst = np.arange(n_dst, dtype=np.float32)
    scale = np.float32(S) / np.float32(n_dst)
    src = scale * (dst + np.float32(0.5)) - np.float32(0.5) if half else scale * dst
    if clamp_src:
        src = np.maximum(src, np.float32(0.0))
    i0 = np.minimum(np.floor(src).astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1) if clamp_i1 else i0 + 1
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    M = np.zeros((n_dst, S + 2), dtype=np.float64)      # column 0: index -1, column S + 1: index S
    rows = np.arange(n_dst)
    np.add.at(M, (rows, i0 + 1), l0.astype(np.float64))
    np.add.at(M, (rows, i1 + 1), l1.astype(np.float64))
    return torch.from_numpy(np.ascontiguousarray(M[:, 1:S + 1]))


def cut_footprint(M, last):
    """the backward gather with the first (last) output row of every source row's footprint missing"""
    M = M.clone()
    for s in range(M.shape[1]):
        nz = torch.nonzero(M[:, s]).flatten()
        if nz.numel():
            M[nz[-1 if last else 0], s] = 0
    return M


def softmax_no_max_fp32(x, dim=-1):
    e = torch.exp(x.float())
    return (e / e.sum(dim=dim, keepdim=True)).to(x.dtype)


def prompt_mutants(case, lg, pp, dout):
    B, L, D, S, H, W, amp = case
    run = lambda: R.prompt_mix(lg, pp, H, W, dout)[0]

    def gather_cut(last):
        w = R.softmax(lg.double(), 1)
        dP = torch.einsum("hs,bdhw,wt->bdst", cut_footprint(R.lerp_matrix(S, H), last), dout.double(), R.lerp_matrix(S, W))
        dw = torch.einsum("bdst,ldst->bl", dP, pp[0].double())
        return {"dparam": torch.einsum("bl,bdst->ldst", w, dP)[None], "dlogits": w * (dw - (w * dw).sum(1, keepdim=True))}

    muts = [("i1_masked", lambda: swapped("lerp_matrix", functools.partial(lerp_variant, clamp_i1=False), run)),
            ("no_half_pixel", lambda: swapped("lerp_matrix", functools.partial(lerp_variant, half=False), run)),
            ("src_not_clamped", lambda: swapped("lerp_matrix", functools.partial(lerp_variant, clamp_src=False), run)),
            ("gather_first_row", lambda: gather_cut(False)), ("gather_last_row", lambda: gather_cut(True))]
    if amp >= 80:
        muts.append(("softmax_no_max", lambda: swapped("softmax", softmax_no_max_fp32, run)))
    return muts


def test_lerp_variant_is_the_restatement():
    for S, n in [(1, 7), (2, 9), (6, 13), (16, 3), (7, 5), (64, 64), (8, 520), (39, 139)]:
        assert torch.equal(lerp_variant(S, n), R.lerp_matrix(S, n)), (S, n)
        assert torch.allclose(R.lerp_matrix(S, n).sum(1), torch.ones(n, dtype=torch.float64), atol=1e-7, rtol=0)


def test_gather_cut_reproduces_the_gradient():
    """the explicit backward the gather mutants are cut from is the autograd gradient when nothing is cut"""
    case = PROMPT_CASES[0]
    lg, pp, dout = prompt_inputs(case)
    ref = R.prompt_mix(lg, pp, case[4], case[5], dout)[0]
    w = R.softmax(lg.double(), 1)
    dP = torch.einsum("hs,bdhw,wt->bdst", R.lerp_matrix(case[3], case[4]), dout.double(), R.lerp_matrix(case[3], case[5]))
    assert rel(torch.einsum("bl,bdst->ldst", w, dP)[None], ref["dparam"]) <= 1e-13


@pytest.mark.parametrize("case", PROMPT_CASES, ids=case_id)
def test_prompt_mix_vs_torch_float64(case):
    """against F.interpolate in float64: apart only by the float32 rounding of the source coordinate, S * 2^-20 of the tensor's scale"""
    B, L, D, S, H, W, amp = case
    lg, pp, dout = prompt_inputs(case)
    out, n = R.prompt_mix(lg, pp, H, W, dout)
    l, p = lg.double().requires_grad_(True), pp.double().requires_grad_(True)
    mixed = (torch.softmax(l, 1)[:, :, None, None, None] * p).sum(1)
    y = F.interpolate(mixed, (H, W), mode="bilinear", align_corners=False)
    y.backward(dout.double())
    tol = S * 2.0 ** -20
    assert rel(out["y"], y) <= tol and rel(out["dlogits"], l.grad) <= tol and rel(out["dparam"], p.grad) <= tol
    fused = R.prompt_mix(lg, pp, H, W, dout, fused=True)[0]       # the coordinate in one FMA: the same distance
    assert rel(fused["y"], y) <= tol and rel(fused["dlogits"], l.grad) <= tol and rel(fused["dparam"], p.grad) <= tol
    A = R.prompt_mix(lg, pp, H, W, dout, absolute=True)[0]
    for k in out:
        assert bool((A[k] * (1 + 1e-12) >= out[k].abs()).all()) and n[k] >= 1, k
    assert bool(((A["dparam"] == 0) == (out["dparam"] == 0)).all())


@pytest.mark.parametrize("case", PROMPT_CASES, ids=case_id)
def test_prompt_mix_case_detects_a_mutation(case):
    B, L, D, S, H, W, amp = case
    lg, pp, dout = prompt_inputs(case)
    ref = R.prompt_mix(lg, pp, H, W, dout)[0]
    big = B * D * H * W > 1 << 20
    hit = detected("prompt", ref, prompt_mutants(case, lg, pp, dout), lazy=big)
    assert any(hit.values()), hit
    if amp >= 100:
        assert hit["softmax_no_max"], hit


def test_prompt_mix_mutations_all_detected_somewhere():
    seen = set()
    for case in PROMPT_CASES:
        if case[0] * case[2] * case[4] * case[5] <= 1 << 16:
            lg, pp, dout = prompt_inputs(case)
            hit = detected("prompt", R.prompt_mix(lg, pp, case[4], case[5], dout)[0], prompt_mutants(case, lg, pp, dout))
            seen |= {k for k, v in hit.items() if v}
    assert seen == {"i1_masked", "no_half_pixel", "src_not_clamped", "gather_first_row", "gather_last_row", "softmax_no_max"}, seen


# ---- mean-pool + linear --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MEANPOOL_CASES, ids=case_id)
def test_meanpool_fc(case):
    B, C, H, W, NC = case
    x, fw, fb, g = meanpool_inputs(case)
    ref, n = R.meanpool_fc(x, fw, fb, g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, fw, fb))
    (xr.sum(dim=(2, 3)) / (H * W) @ wr.t() + br).backward(g.double())
    assert rel(ref["dx"], xr.grad) <= 1e-12 and rel(ref["dfw"], wr.grad) <= 1e-12 and rel(ref["dfb"], br.grad) <= 1e-12
    assert rel(ref["logits"], xr.detach().sum(dim=(2, 3)) / (H * W) @ wr.detach().t() + br.detach()) <= 1e-12
    A = R.meanpool_fc(x, fw, fb, g, absolute=True)[0]
    assert all(bool((A[k] * (1 + 1e-12) >= ref[k].abs()).all()) for k in ref)
    # sensitivity: the last pixel (of the last slice) dropped; the divisor per * nsl instead of P
    P = H * W
    nsl, per = pool_slices(P)
    xcut = x.clone()
    xcut[..., -1, -1] = 0
    hit = detected("meanpool", ref, [("last_pixel_dropped", lambda: R.meanpool_fc(xcut, fw, fb, g)[0]),
                                     ("divisor_per_nsl", lambda: R.meanpool_fc(x * (P / (per * nsl)), fw, fb, g)[0])])
    assert any(hit.values()), hit
    if per * nsl != P:
        assert hit["divisor_per_nsl"], hit


def test_meanpool_cases_cover_the_slice_geometry():
    """what the sizes were chosen for: one slice below P = 128; a last slice of 2 .. 5 pixels at 63 / 64 / 64 slices"""
    geo = {c[2] * c[3]: pool_slices(c[2] * c[3]) for c in MEANPOOL_CASES}
    assert [geo[p][0] for p in (1, 63, 64, 127)] == [1, 1, 1, 1] and geo[128][0] == 2 and geo[130] == (2, 65) and geo[191] == (2, 96)
    last = {p: p - (geo[p][0] - 1) * geo[p][1] for p in (4033, 4097, 4100)}
    assert [geo[p][0] for p in (4033, 4097, 4100)] == [63, 64, 64] and last == {4033: 3, 4097: 2, 4100: 5}


# ---- conv1x1 -> pool -> ReLU ---------------------------------------------------------------------------------------------------
def route_variant(vs, last=False, ge=False, relu=True, three=False):
    m, idx = vs[0], torch.zeros(vs[0].shape, dtype=torch.int64)
    for k in (1, 2) if three else (1, 2, 3):
        up = vs[k] >= m if last else vs[k] > m
        m = torch.where(up, vs[k], m)
        idx = torch.where(up, torch.full_like(idx, k), idx)
    return idx, (torch.ones_like(m, dtype=torch.bool) if not relu else (m >= 0 if ge else m > 0))


def pool_mutants(x, w, dy):
    run = lambda: R.conv1x1_pool_relu(x, w, dy)[0]
    # (the first two are the mistakes the kernel's comment rules out; they show only on ties and on zero maxima, so the random cases
    # are held to two plainer ones: no ReLU, and a window that ends after three elements)
    return [("no_relu", lambda: swapped("route", functools.partial(route_variant, relu=False), run)),
            ("last_maximum", lambda: swapped("route", functools.partial(route_variant, last=True), run)),
            ("ge_zero", lambda: swapped("route", functools.partial(route_variant, ge=True), run)),
            ("three_of_four", lambda: swapped("route", functools.partial(route_variant, three=True), run))]


POOL_ALL = POOL_RANDOM + POOL_SPECIAL


@pytest.mark.parametrize("case", POOL_ALL, ids=case_id)
def test_conv1x1_pool_relu(case):
    """against F.max_pool2d in float64 -- on the tie cases this is the statement that torch routes to the first maximum in scan order"""
    x, w, dy = pool_inputs(case)
    ref, n = R.conv1x1_pool_relu(x, w, dy)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.relu(F.max_pool2d(F.conv2d(xr, wr), 2, 2))
    y.backward(dy.double())
    assert rel(ref["y"], y) <= 1e-12 and rel(ref["dx"], xr.grad) <= 1e-12 and rel(ref["dw"], wr.grad) <= 1e-12
    z = ref["z"]
    a, b, c, d = R.windows(z)
    if case == "quad" or case == "const":
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d), "equal pixels must give bit-equal conv outputs"
    elif case == "top":
        assert torch.equal(a, b)
    elif case == "left":
        assert torch.equal(a, c)
    elif case == "neg":
        assert bool((z < 0).all()) and not ref["y"].any() and not ref["dx"].any() and not ref["dw"].any()
    elif case == "zero":
        assert not z.any() and not ref["y"].any() and not ref["dx"].any() and not ref["dw"].any()
    else:
        share = float(R.ambiguous_windows(z).double().mean())
        print(f"pool {case}: excluded share {share:.3e}")
        assert share <= 1e-3
    A = R.conv1x1_pool_relu(x, w, dy, absolute=True)[0]
    assert all(bool((A[k] * (1 + 1e-12) >= ref[k].abs()).all()) for k in ("y", "dx", "dw"))
    hit = detected("pool", ref, pool_mutants(x, w, dy), lazy=z.numel() > 1 << 20)
    assert any(hit.values()), hit
    if case in ("quad", "top", "left", "const"):
        assert hit["last_maximum"], hit
    if case == "zero":
        assert hit["ge_zero"], hit


# ---- dense mix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MIX_CASES, ids=case_id)
@pytest.mark.parametrize("use_prev", [True, False])
def test_mix(case, use_prev):
    shape, n, idx, amp = case
    prev, feat, mw, go = mix_inputs(case)
    prev = prev if use_prev else None
    ref, _ = R.mix(prev, feat, mw, idx, go)
    fr, mr = feat.double().requires_grad_(True), mw.double().requires_grad_(True)
    pr = prev.double().requires_grad_(True) if use_prev else None
    y = torch.softmax(mr, 0)[idx] * fr + (pr if use_prev else 0)
    y.backward(go.double())
    assert rel(ref["y"], y) <= 1e-12 and rel(ref["dfeat"], fr.grad) <= 1e-12
    A = R.mix(prev, feat, mw, idx, go, absolute=True)[0]
    # dmix = ds s_i (delta_ij - s_j): where s_idx is all but 1 (the +-50 case) the whole vector is a cancelled difference, and two float64
    # evaluations agree to the float64 resolution of its magnitude sum A (16 x 2^-53 of it), not to 1e-12 of its own scale
    assert float((ref["dmix"] - mr.grad).abs().max()) <= max(1e-12 * float(mr.grad.abs().max()), 2.0 ** -49 * float(A["dmix"].max()))
    if use_prev:
        assert torch.equal(ref["dprev"], go.double())
    if n == 1:
        assert not ref["dmix"].any()
    assert all(bool((A[k] * (1 + 1e-12) >= ref[k].abs()).all()) for k in ref)

    def no_sj():
        s = R.softmax(mw.double(), 0)
        onehot = torch.zeros_like(s)
        onehot[idx] = 1
        return {"dmix": (go.double() * feat.double()).sum() * s[idx] * onehot}

    hit = detected("mix", ref, [("idx_off_by_one", lambda: R.mix(prev, feat, mw, (idx + 1) % n, go)[0]), ("dmix_without_sj", no_sj)])
    assert any(hit.values()), hit


# ---- image embedding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EMBED_SHAPES, ids=case_id)
def test_conv_embed_ln(shape):
    ts = embed_inputs(shape)
    ref, n = R.conv_embed_ln(*ts)
    x, w, b, lw, lb = (t.double().requires_grad_(True) for t in ts[:5])
    z = F.conv2d(x, w, b, stride=2, padding=3)
    y = F.layer_norm(z.permute(0, 2, 3, 1), (EMBED_DIM,), lw, lb, eps=1e-6).permute(0, 3, 1, 2)
    y.backward(ts[5].double())
    assert rel(ref["y"], y) <= 1e-12
    for k, t in zip(("dx", "dw", "db", "dlnw", "dlnb"), (x, w, b, lw, lb)):
        assert rel(ref[k], t.grad) <= 1e-12, k
    A = R.conv_embed_ln(*ts, absolute=True)[0]
    assert all(bool((A[k] * (1 + 1e-12) >= ref[k].abs()).all()) for k in ref)
