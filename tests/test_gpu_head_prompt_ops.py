"""GPU: the glue kernels of the PromptIR prompt block (promptir.hip) and of the degradation-classifier head (dchead.hip: mean-pool +
linear, conv1x1 -> max-pool -> ReLU, the dense mix, the image embedding's unfold / fold), op by op through the public functions against
the kernel-blind float64 restatements of tests/head_prompt_restatement.py.  Cases and inputs: tests/test_head_prompt_restatement_cpu.py,
which also shows that every case tells a deliberate index mistake from the restatement.

Every fp32 output is held to two checks.  The scale-relative max error the project already uses for the op (TOL), and per element
    |got - ref| <= 4 * max(r_cpu, u * sqrt(n)) * A        (+ 4 * 2^-126: a result below fp32's smallest normal may be flushed)
with u = 2^-24, A the element's magnitude sum and n its count of summed terms from the restatement, and r_cpu the largest
|fp32 - fp64| / A of the restatement itself evaluated in torch fp32 on the CPU -- from the reference alone, never from the kernel.  The
factor 4 is for summation order and FMA contraction.  Elements far below the tensor's maximum, which a scale-relative number never sees,
are checked by this.  (r_cpu and the kernel's own ratio are taken over the elements with A >= 2^-100: below that fp32 products of the
terms are subnormal and their relative error says nothing.)"""
import math

import pytest
import torch
import torch.nn.functional as F

import head_prompt_restatement as R
import tests.test_head_prompt_restatement_cpu as C
from kernel_trace import kernel_trace

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TINY = 2.0 ** -100


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def nhwc(t):
    """dense NHWC memory whatever the extents (channels_last is ambiguous at C = 1 or H * W = 1)"""
    n, c, h, w = t.shape
    out = torch.empty_strided((n, c, h, w), (h * w * c, 1, w * c, c), dtype=t.dtype, device=t.device)
    return out.copy_(t)


def element_bound(k, ref, A, n, r32):
    """-> (the per-element bound of the module docstring for output k, r_cpu, u sqrt(n))"""
    r, a = ref[k].double(), A[k].double()
    big = a >= TINY
    r_cpu = float(((r32[k].double() - r).abs()[big] / a[big]).max()) if bool(big.any()) else 0.0
    floor = U * math.sqrt(n[k])
    return 4 * max(r_cpu, floor) * a + 4 * 2.0 ** -126, r_cpu, floor


def compare(op, case, got, ref, A, n, r32, alt=None):
    """both checks of the module docstring on every tensor of ``got``.  ``alt``: a second legitimate fp32 evaluation of the reference;
    an element meets the per-element bound against either (the scale-relative check is against ``ref`` alone)."""
    bad = []
    for k, t in got.items():
        g, r, a = t.detach().float().cpu().double(), ref[k].double(), A[k].double()
        assert g.shape == r.shape == a.shape, (k, g.shape, r.shape, a.shape)
        err = (g - r).abs()
        e = float(err.max()) / max(float(r.abs().max()), 1e-30)
        bound, r_cpu, floor = element_bound(k, ref, A, n, r32)
        big = a >= TINY
        ratio = lambda d: float((d[big] / a[big]).max()) if bool(big.any()) else 0.0
        r_hip = ratio(err)
        note = ""
        if alt is not None:
            err = torch.minimum(err, (g - alt[k].double()).abs())
            note = f" ({ratio(err):.3e} against the nearer of the two coordinate forms)"
        print(f"[head_prompt] {op} {C.case_id(case)} {k}: scale-relative {e:.3e} (tol {C.TOL[op][k]:.0e}); per element kernel {r_hip:.3e}{note}, "
              f"r_cpu {r_cpu:.3e}, u sqrt(n) {floor:.3e}")
        if not (math.isfinite(e) and e <= C.TOL[op][k]):
            bad.append(f"{k}: scale-relative max error {e:.3e} > {C.TOL[op][k]:.0e}")
        if not bool((err <= bound).all()):
            bad.append(f"{k}: |got - ref| / A reaches {ratio(err):.3e} > 4 * max(r_cpu {r_cpu:.3e}, u sqrt(n) {floor:.3e})")
    assert not bad, f"{op} {C.case_id(case)}: " + "; ".join(bad)


def bf16_within_one_ulp(name, got, ref, slack=None):
    """a bf16 result against the float64 reference rounded to bf16.  ``slack``: the per-element fp32 bound of the value that is rounded,
    where the op's result can cancel (there one bf16 ulp of the result is less than the fp32 error of its terms)."""
    assert got.dtype == torch.bfloat16, name
    rb = ref.float().bfloat16().double()
    _, ex = torch.frexp(rb.abs())
    ulp = torch.ldexp(torch.ones_like(rb), ex - 8)
    ulp[rb == 0] = 0
    if slack is not None:
        ulp = ulp + slack
    d = (got.detach().cpu().double() - rb).abs()
    assert bool((d <= ulp).all()), f"{name}: {int((d > ulp).sum())} elements more than one bf16 ulp from the rounded reference"


# ---- prompt mix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.PROMPT_CASES, ids=C.case_id)
def test_prompt_mix(dev, case):
    from dcpt_amd import functional as DF

    B, L, D, S, H, W, amp = case
    lg, pp, dout = C.prompt_inputs(case)
    ref, n = R.prompt_mix(lg, pp, H, W, dout)
    A = R.prompt_mix(lg, pp, H, W, dout, absolute=True)[0]
    r32 = R.prompt_mix(lg, pp, H, W, dout, dtype=torch.float32)[0]

    def run(bf):
        l, p = lg.to(dev).requires_grad_(True), pp.to(dev).requires_grad_(True)
        y = DF.prompt_mix(l, p, H, W, out_bf16=bf)
        assert y.dtype == (torch.bfloat16 if bf else torch.float32) and tuple(y.shape) == (B, D, H, W)
        y.backward(dout.to(dev).bfloat16() if bf else dout.to(dev))
        return {"y": y.detach(), "dlogits": l.grad, "dparam": p.grad}

    got = run(False)
    # The kernel's source coordinate is one FMA (the compiler contracts scale * (dst + 0.5) - 0.5); against the two-rounding form of the
    # restatement alone the per-element ratio reached 3.5e-6 (y) and 7.1e-6 (dparam) at (1, 5, 128, 32, 40, 24), 11x and 20x the rate,
    # against the fused form 2.1e-7 and 3.5e-7.  Both are float32 evaluations of the stated formula: an element may match either.
    compare("prompt", case, got, ref, A, n, r32, alt=R.prompt_mix(lg, pp, H, W, dout, fused=True)[0])
    outside = ref["dparam"] == 0          # source pixels outside every footprint (down-scaling)
    assert not bool(got["dparam"].cpu()[outside].any()), "a source pixel outside every bilinear footprint has a gradient"
    if D % 8 == 0:
        # the bf16 map is the fp32 kernel with one rounding on store (test_prompt_mix_bf16_is_fp32_rounded, on these geometries)
        with kernel_trace() as tr:
            gb = run(True)
        assert tr["prompt_bf16.mix"] == 2, tr.counts
        assert torch.equal(gb["y"], got["y"].bfloat16())
        assert torch.equal(gb["dlogits"], got["dlogits"]) and torch.equal(gb["dparam"], got["dparam"])


# ---- mean-pool + linear --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MEANPOOL_CASES, ids=C.case_id)
@pytest.mark.parametrize("bias", [True, False])
def test_meanpool_fc(dev, case, bias):
    from dcpt_amd import functional as DF

    x, fw, fb, g = C.meanpool_inputs(case)
    fb = fb if bias else None
    for bf in (False, True):
        xin = x.bfloat16().float() if bf else x          # bf16 storage: the reference sees the rounded input
        ref, n = R.meanpool_fc(xin, fw, fb, g)
        A = R.meanpool_fc(xin, fw, fb, g, absolute=True)[0]
        r32 = R.meanpool_fc(xin, fw, fb, g, dtype=torch.float32)[0]
        xg = nhwc(xin.to(dev).bfloat16() if bf else xin.to(dev)).requires_grad_(True)
        wg = fw.to(dev).requires_grad_(True)
        bg = fb.to(dev).requires_grad_(True) if bias else None
        logits = DF.meanpool_fc(xg, wg, bg)
        logits.backward(g.to(dev))
        got = {"logits": logits.detach(), "dfw": wg.grad}
        if bias:
            got["dfb"] = bg.grad
        if bf:
            bf16_within_one_ulp("dx", xg.grad, ref["dx"])
        else:
            got["dx"] = xg.grad
        compare("meanpool", case + (("bias",) if bias else ()) + (("bf16",) if bf else ()), got, ref, A, n, r32)


# ---- conv1x1 -> max-pool -> ReLU -----------------------------------------------------------------------------------------------
def _pool_fp32(dev, x, w, dy):
    from dcpt_amd import functional as DF

    xg, wg = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    y = DF.conv1x1_pool_relu(xg, wg)
    y.backward(dy.to(dev))
    return {"y": y.detach(), "dx": xg.grad, "dw": wg.grad}


@pytest.mark.parametrize("case", C.POOL_RANDOM, ids=C.case_id)
def test_conv1x1_pool_relu_random(dev, case):
    """windows whose routing a last-bit difference of z could change take no gradient, on both sides; their share is bounded"""
    x, w, dy = C.pool_inputs(case)
    amb = R.ambiguous_windows(R.conv1x1_pool_relu(x, w)[0]["z"])
    share = float(amb.double().mean())
    print(f"[head_prompt] pool {C.case_id(case)}: excluded windows {int(amb.sum())} of {amb.numel()} = {share:.3e}")
    assert share <= 1e-3
    dy = dy * (~amb)
    ref, n = R.conv1x1_pool_relu(x, w, dy)
    A = R.conv1x1_pool_relu(x, w, dy, absolute=True)[0]
    r32 = R.conv1x1_pool_relu(x, w, dy, dtype=torch.float32)[0]
    compare("pool", case, _pool_fp32(dev, x, w, dy), ref, A, n, r32)


@pytest.mark.parametrize("case", C.POOL_SPECIAL)
def test_conv1x1_pool_relu_ties_and_signs(dev, case):
    """exact ties (equal pixels in a window: flat image regions) go to the first maximum in scan order like F.max_pool2d on the CPU; a
    window whose maximum is <= 0 passes nothing, exactly"""
    from dcpt_amd import functional as DF
    from oracle.nafnet_oracle import _rb, _rf, _rr

    x, w, dy = C.pool_inputs(case)
    z = R.conv1x1_pool_relu(x, w)[0]["z"]
    dyf = dy * (~R.ambiguous_windows(z, exact_ties_count=False))      # near-ties of DIFFERENT pixels are not the subject
    ref, n = R.conv1x1_pool_relu(x, w, dyf)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.relu(F.max_pool2d(F.conv2d(xr, wr), 2, 2))
    yr.backward(dyf.double())
    assert C.rel(ref["y"], yr) <= 1e-12 and C.rel(ref["dx"], xr.grad) <= 1e-12 and C.rel(ref["dw"], wr.grad) <= 1e-12
    A = R.conv1x1_pool_relu(x, w, dyf, absolute=True)[0]
    r32 = R.conv1x1_pool_relu(x, w, dyf, dtype=torch.float32)[0]
    got = _pool_fp32(dev, x, w, dyf)
    compare("pool", case, got, ref, A, n, r32)
    if case in ("neg", "zero"):
        assert not any(bool(t.any()) for t in got.values()), "y, dx and dw are exactly 0 when no window maximum is > 0"
    # bf16 storage against the bf16-emulating reference of test_conv1x1_pool_relu_bf16_oracle (same 2e-2).  The stored z is rounded to
    # bf16, which makes ties of its own: windows whose two largest DIFFERENT values lie within 2^-6 of max|z| take no gradient.
    xb, dyb = x.bfloat16().float(), dy.bfloat16().float()
    dyb = dyb * (~R.ambiguous_windows(R.conv1x1_pool_relu(xb, w.bfloat16().float())[0]["z"], rel=2.0 ** -6, exact_ties_count=False))
    xe, we = xb.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ye = _rr(F.relu(F.max_pool2d(_rr(F.conv2d(_rb(xe), _rf(we))), 2, 2)))
    (ye * dyb).sum().backward()
    xd, wd = nhwc(xb.to(dev).bfloat16()).requires_grad_(True), w.to(dev).requires_grad_(True)
    yd = DF.conv1x1_pool_relu_bf16(xd, wd)
    yd.backward(dyb.to(dev).bfloat16())
    if case in ("neg", "zero"):
        assert not bool(yd.any()) and not bool(xd.grad.any()) and not bool(wd.grad.any())
    errs = {"y": _rel(yd, ye), "dx": _rel(xd.grad, xe.grad), "dw": _rel(wd.grad, we.grad)}
    assert all(math.isfinite(v) and v <= 2e-2 for v in errs.values()), errs


def _rel(a, b):
    a, b = a.detach().float().cpu().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# ---- dense mix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MIX_CASES, ids=C.case_id)
@pytest.mark.parametrize("use_prev", [True, False])
def test_mix(dev, case, use_prev):
    from dcpt_amd import functional as DF

    shape, nw, idx, amp = case
    prev, feat, mw, go = C.mix_inputs(case)
    for bf in (False, True):
        rnd = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
        pi, fi, gi = (rnd(prev) if use_prev else None), rnd(feat), rnd(go)
        ref, n = R.mix(pi, fi, mw, idx, gi)
        A = R.mix(pi, fi, mw, idx, gi, absolute=True)[0]
        r32 = R.mix(pi, fi, mw, idx, gi, dtype=torch.float32)[0]
        put = lambda t: nhwc(t.to(dev).bfloat16() if bf else t.to(dev))
        pg = put(pi).requires_grad_(True) if use_prev else None
        fg, mg = put(fi).requires_grad_(True), mw.to(dev).requires_grad_(True)
        with kernel_trace() as tr:
            y = DF.mix(pg, fg, mg, idx)
            y.backward(put(gi))
        tr.assert_not_ran("head.mix_stride_fwd", "head.mix_stride_bwd")      # the dense kernels
        got = {"dmix": mg.grad}
        if bf:
            # (prev + s * feat cancels to exactly 0 in fp32 where the reference, whose s is not rounded to 1, keeps 5e-9 * feat)
            bf16_within_one_ulp("y", y, ref["y"], slack=element_bound("y", ref, A, n, r32)[0])
            bf16_within_one_ulp("dfeat", fg.grad, ref["dfeat"])
            if use_prev:
                assert torch.equal(pg.grad.cpu().float(), gi), "dprev is dout"
        else:
            got.update(y=y.detach(), dfeat=fg.grad)
            if use_prev:
                got["dprev"] = pg.grad
        compare("mix", case + (("prev",) if use_prev else ()) + (("bf16",) if bf else ()), got, ref, A, n, r32)
        if nw == 1:
            assert not bool(mg.grad.any()), "one mixing weight: s = 1 and dmix = 0 exactly"


# ---- image embedding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.EMBED_SHAPES, ids=C.case_id)
def test_conv_embed_ln(dev, shape):
    from dcpt_amd import functional as DF

    ts = C.embed_inputs(shape)
    ref, n = R.conv_embed_ln(*ts)
    A = R.conv_embed_ln(*ts, absolute=True)[0]
    r32 = R.conv_embed_ln(*ts, dtype=torch.float32)[0]
    x, w, b, lw, lb = (t.to(dev).requires_grad_(True) for t in ts[:5])
    y = DF.conv_embed_ln(x, w, b, lw, lb)
    assert tuple(y.shape) == tuple(ref["y"].shape)
    y.backward(ts[5].to(dev))
    got = {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad, "dlnw": lw.grad, "dlnb": lb.grad}
    compare("embed", shape, got, ref, A, n, r32)
