"""The fused step tail on the GPU: dcpt_amd.optim.FusedAdamW.step(max_grad_norm=, ema=) (include/dcpt_hip.h dcpt_grad_norm /
dcpt_adamw_step_ex) against the three calls it replaces (reference sr_model.py:166-174: clip_grad_norm_, optimizer.step(), model_ema();
base_model.py:86-95), and ``train.fused_step_tail`` of SRModel / DCDistModel.

The parameter list is the zoo of test_gpu_optim.py plus what crosses every boundary of the kernels: channels-last 4-D tensors, 4-byte-offset
views of one buffer (the scalar path), an empty tensor, 170 tensors of 1-33 elements (three launches of 80 tensors) and one parameter
without a gradient (the EMA fallback)."""
import ctypes as C

import numpy as np
import pytest
import torch

from kernel_trace import kernel_trace

pytestmark = pytest.mark.gpu

SHAPES = [(7,), (64,), (1, 64, 1, 1), (128, 64, 1, 1), (64, 1, 3, 3), (4099,), (3, 5, 7), (512, 512), (2, 4097)]
GRAD_CLIP = 1e-3   # of the model tests: far below the gradient norm of one L1 step
NOGRAD = len(SHAPES) + 2 + 2 + 1 + 170   # index of the parameter that never gets a gradient
DECAY = 0.9


def _zoo(dev, seed=0):
    """(parameters, EMA copies).  The EMA copy of the second channels-last parameter is row-major: it cannot ride in the kernel."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ts = [torch.randn(s, generator=g).to(dev) for s in SHAPES]
    ts += [torch.randn(s, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for s in [(32, 16, 3, 3), (8, 24, 5, 5)]]
    base = torch.randn(1 + 4099 + 64, generator=g).to(dev)
    ts += [base[1:1 + 4099], base[1 + 4099:]]
    ts += [torch.zeros(0, device=dev)]
    ts += [torch.randn(1 + i % 33, generator=g).to(dev) for i in range(170)]
    ts += [torch.randn(5, generator=g).to(dev)]
    ps = [torch.nn.Parameter(t) for t in ts]
    es = [torch.empty_like(p).copy_(p.detach() + 0.1 * torch.randn(p.shape, generator=g).to(dev)) for p in ps]   # (the parameter's layout)
    k = len(SHAPES) + 1
    es[k] = es[k].contiguous()
    assert es[k].stride() != ps[k].stride() and es[k - 1].stride() == ps[k - 1].stride() and len(ps) == NOGRAD + 1
    return ps, es


def _grads(ps, seed, scale=0.1, zero=False):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    for i, p in enumerate(ps):
        if i == NOGRAD:
            p.grad = None
            continue
        gr = (torch.randn(p.shape, generator=g) * scale * (0.0 if zero else 1.0)).to(p.device)
        p.grad = gr.contiguous(memory_format=torch.channels_last) if p.dim() == 4 and not p.is_contiguous() else gr


def _host_norm(ps):
    return float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in ps if p.grad is not None)).cpu())


def _fused(ps, **kw):
    from dcpt_amd.optim import FusedAdamW

    return FusedAdamW(ps, **kw)


def _bits(ts):
    return [t.detach().clone().view(torch.int32) if t.numel() else t.detach().clone() for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. the norm -----------------------------------------------------------------------------------------------------------------------

def test_grad_norm_matches_the_host_in_double_and_repeats_bit_for_bit():
    dev = torch.device("cuda", 0)
    ps, _ = _zoo(dev)
    opt = _fused(ps, lr=1e-3)
    _grads(ps, 0)
    want = _host_norm(ps)
    with kernel_trace() as t:
        opt.step(max_grad_norm=1.0)
    assert t["grad_norm.sumsq"] == 3 and t["grad_norm.finish"] == 1 and t["adamw.clip"] == 3   # 183 non-empty tensors, 80 per launch
    n1 = opt.grad_norm.clone()
    assert n1.shape == (1,) and n1.dtype == torch.float32 and n1.is_cuda
    rel = abs(float(n1.double().cpu()) - want) / want
    print(f"grad_norm {float(n1):.9g} host {want:.17g} rel {rel:.3e}")
    # fp64 accumulation contributes nothing visible; one rounding to fp32 after the square root
    assert rel <= 2.0 ** -23
    opt.step(max_grad_norm=1.0)   # the gradients are not scaled in place: the same norm again, to the bit
    assert torch.equal(opt.grad_norm.view(torch.int32), n1.view(torch.int32))


def test_grad_norm_of_zero_and_of_nothing_is_zero_with_coefficient_one():
    from dcpt_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    gs = [torch.zeros(5000, device=dev), torch.zeros(0, device=dev), torch.zeros(3, device=dev)]
    numel = (C.c_int64 * 3)(*[g.numel() for g in gs])
    need = lib.dcpt_grad_norm_ws_bytes(3, numel)
    assert need == 8 * 3
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    out = torch.full((2,), 7.0, device=dev)
    _lib.check(lib.dcpt_grad_norm(3, (C.c_void_p * 3)(*[g.data_ptr() for g in gs]), numel, 0.5, ws.data_ptr(), need, out.data_ptr(), stream))
    assert out.tolist() == [0.0, 1.0]
    out.fill_(7.0)
    with kernel_trace() as t:   # every tensor empty: no sum-of-squares launch, the finisher still writes {0, 1}
        _lib.check(lib.dcpt_grad_norm(1, (C.c_void_p * 1)(None), (C.c_int64 * 1)(0), 0.5, None, 0, out.data_ptr(), stream))
    assert out.tolist() == [0.0, 1.0] and t["grad_norm.sumsq"] == 0 and t["grad_norm.finish"] == 1
    ps, _ = _zoo(dev)
    opt = _fused(ps, lr=1e-3)
    _grads(ps, 0, zero=True)
    opt.step(max_grad_norm=0.5)
    assert float(opt.grad_norm) == 0.0


# ---- 2. coefficient 1 / no EMA: the plain step, bit for bit --------------------------------------------------------------------------------

@pytest.mark.parametrize("with_ema", [False, True])
def test_unclipped_fused_step_is_the_plain_step_bit_for_bit(with_ema):
    dev = torch.device("cuda", 0)
    kw = dict(lr=3e-4, betas=(0.9, 0.999), weight_decay=1e-2)
    a, ea = _zoo(dev)
    b, _ = _zoo(dev)
    oa, ob = _fused(a, **kw), _fused(b, **kw)
    ema = (dict(zip(a, ea)), DECAY) if with_ema else None
    for step in range(3):
        _grads(a, step)
        _grads(b, step)
        oa.step(max_grad_norm=1e30, ema=ema)   # far above the norm: the coefficient is exactly 1 and g * 1.0f is exact
        ob.step()
        assert float(oa.grad_norm) < 1e30
        assert _same_bits(_bits(a), _bits(b))
        for key in ("exp_avg", "exp_avg_sq"):
            assert _same_bits(_bits([oa.state[p][key] for p in a[:NOGRAD]]), _bits([ob.state[p][key] for p in b[:NOGRAD]]))
    if with_ema:   # ema=(...) alone, no clipping: the same again
        oa.step(ema=ema)
        ob.step()
        assert _same_bits(_bits(a), _bits(b))


# ---- 3. clipping and the EMA are visible, and as accurate as torch's ---------------------------------------------------------------------------

KW3 = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-3, weight_decay=1e-2)   # eps as large as the clipped gradients: Adam's scale invariance is off
STEPS3 = 4


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def _truth_step(P, M, V, E, grads, t, max_norm):
    """float64 host evaluation of ONE clip -> AdamW -> EMA step from the fp32 inputs given as float64 CPU tensors (``grads[i]`` None: no
    gradient); the coefficient rounded to fp32 the way both implementations hold it.  Returns ([p], [exp_avg], [exp_avg_sq], [ema])."""
    b1, b2 = KW3["betas"]
    norm = np.float32(float(torch.sqrt(sum(g.pow(2).sum() for g in grads if g is not None))))
    c = np.float32(max_norm) / (norm + np.float32(1e-6))
    coef = float(np.float32(1.0) if c > 1.0 else c)
    assert 0.005 < coef < 0.02   # about 0.01: the clip bites
    P, M, V, E = list(P), list(M), list(V), list(E)
    for i, g in enumerate(grads):
        if g is not None:
            g = g * coef
            P[i] = P[i] - KW3["lr"] * KW3["weight_decay"] * P[i]
            M[i] = M[i] + (1 - b1) * (g - M[i])
            V[i] = b2 * V[i] + (1 - b2) * g * g
            P[i] = P[i] - (KW3["lr"] / (1 - b1 ** t)) * M[i] / (V[i].sqrt() / (1 - b2 ** t) ** 0.5 + KW3["eps"])
        E[i] = DECAY * E[i] + (1 - DECAY) * P[i]
    return P, M, V, E


def _f64(ts):
    return [t.detach().double().cpu() for t in ts]


def _moments(opt, ps, key):
    return [opt.state[p][key] if key in opt.state[p] else torch.zeros_like(p) for p in ps]


def test_clipped_step_with_ema_is_as_accurate_as_the_torch_route():
    """err_hip <= 2 * err_ref + one fp32 ulp of the tensor's largest magnitude, per tensor, for p / exp_avg / exp_avg_sq / EMA, over 4 steps.
    err_ref: clip_grad_norm_ + torch.optim.AdamW + the foreach pair on the GPU; both against a float64 host evaluation FROM THE SAME fp32
    INPUTS: before every step the torch route is handed the fused route's parameters, moments and EMA copies, and the float64 evaluation
    starts from them too, so each of the 4 steps (bias corrections of t = 1 .. 4, moments and EMA with history) compares three evaluations
    of one step from identical inputs.  Measured on an MI355X, worst tensor over the 4 steps in ulps of its largest magnitude, fused / torch
    route: p 0.99 / 1.19, exp_avg 3.9 / 6.7, exp_avg_sq 2.6 / 4.0, EMA 1.25 / 1.27.  (Letting the three run free instead compares
    rounding histories -- some six independent roundings of +-0.5 ulp per parameter and route after three steps, the tail of which some
    of the 170 tiny tensors always reach: measured that way the fused route was over twice the torch route's error + 1 ulp in 1 tensor
    and the torch route over twice the fused route's + 1 ulp in 28.)"""
    dev, cpu = torch.device("cuda", 0), torch.device("cpu")
    a, ea = _zoo(dev)
    b, eb = _zoo(dev)
    host_ps, _ = _zoo(cpu)   # (the gradients once more on the host, for the float64 evaluation)
    oa, ob = _fused(a, **KW3), torch.optim.AdamW(b, **KW3)
    ema = (dict(zip(a, ea)), DECAY)
    _grads(host_ps, 0)
    max_norm = 0.01 * _host_norm(host_ps)   # coefficient about 0.01
    worst = {}
    for step in range(STEPS3):
        _grads(a, step)
        _grads(b, step)
        _grads(host_ps, step)
        with torch.no_grad():   # the same fp32 inputs for the torch route ...
            for x, y in zip(a, b):
                y.copy_(x)
            for key in ("exp_avg", "exp_avg_sq"):
                if step > 0:
                    for x, y in zip(_moments(oa, a, key), _moments(ob, b, key)):
                        y.copy_(x)
            for x, y in zip(ea, eb):
                y.copy_(x)
        # ... and for the float64 evaluation
        truth = _truth_step(_f64(a), _f64(_moments(oa, a, "exp_avg")), _f64(_moments(oa, a, "exp_avg_sq")), _f64(ea),
                            [None if p.grad is None else p.grad.double() for p in host_ps], step + 1, max_norm)
        oa.step(max_grad_norm=max_norm, ema=ema)
        torch.nn.utils.clip_grad_norm_(b, max_norm)
        ob.step()
        torch._foreach_mul_(eb, DECAY)
        torch._foreach_add_(eb, [p.detach() for p in b], alpha=1 - DECAY)
        for name, want, hip, ref in (("p", truth[0], a, b), ("exp_avg", truth[1], _moments(oa, a, "exp_avg"), _moments(ob, b, "exp_avg")),
                                     ("exp_avg_sq", truth[2], _moments(oa, a, "exp_avg_sq"), _moments(ob, b, "exp_avg_sq")),
                                     ("ema", truth[3], ea, eb)):
            bad = []
            for i, (w, x, y) in enumerate(zip(want, _f64(hip), _f64(ref))):
                if w.numel() == 0:
                    continue
                err_hip, err_ref = float((x - w).abs().max()), float((y - w).abs().max())
                ulp = _ulp(float(w.abs().max()))
                for k, e in (((name, "hip/ulp"), err_hip), ((name, "ref/ulp"), err_ref)):
                    worst[k] = max(worst.get(k, 0.0), e / ulp)
                if not err_hip <= 2 * err_ref + ulp:
                    bad.append((step, name, i, tuple(w.shape), err_hip, err_ref, ulp))
            print(f"step {step} {name}: worst so far hip {worst[(name, 'hip/ulp')]:.3f} ref {worst[(name, 'ref/ulp')]:.3f} ulp, {len(bad)} over the bound")
            assert not bad, bad[:5]


# ---- 4. the gradient is untouched; the parameter without a gradient ---------------------------------------------------------------------------

def test_gradients_stay_unscaled_and_the_ema_fallback_moves_what_the_kernel_does_not():
    dev = torch.device("cuda", 0)
    a, ea = _zoo(dev)
    opt = _fused(a, **KW3)
    _grads(a, 0)
    before_g = _bits([p.grad for p in a[:NOGRAD]])
    before_p, before_e = [p.detach().clone() for p in a], [e.clone() for e in ea]
    versions = [e._version for e in ea]
    with kernel_trace() as t:
        opt.step(max_grad_norm=0.01 * _host_norm(a), ema=(dict(zip(a, ea)), DECAY))
    assert t["adamw.clip_ema"] == 3 and t["adamw.clip"] == 1   # (the row-major EMA copy of a channels-last parameter: stepped without it)
    assert _same_bits(_bits([p.grad for p in a[:NOGRAD]]), before_g)
    assert torch.equal(a[NOGRAD].detach(), before_p[NOGRAD])
    k = len(SHAPES) + 1
    for i in (NOGRAD, k):   # the foreach pair over exactly these two
        want = (before_e[i] * DECAY).add(a[i].detach(), alpha=1 - DECAY)
        torch.testing.assert_close(ea[i], want, rtol=1e-6, atol=1e-7)
        assert not torch.equal(ea[i], before_e[i])
    assert not torch.equal(a[k].detach(), before_p[k])
    assert all(e._version > v for e, v in zip(ea, versions) if e.numel())


# ---- 5. a NaN gradient ---------------------------------------------------------------------------------------------------------------------

def test_a_nan_gradient_gives_a_nan_norm_and_nan_parameters_on_both_routes():
    dev = torch.device("cuda", 0)
    a, ea = _zoo(dev)
    b, _ = _zoo(dev)
    oa, ob = _fused(a, **KW3), torch.optim.AdamW(b, **KW3)
    for ps in (a, b):
        _grads(ps, 0)
        ps[5].grad[17] = float("nan")
    oa.step(max_grad_norm=1.0, ema=(dict(zip(a, ea)), DECAY))
    ref_norm = torch.nn.utils.clip_grad_norm_(b, 1.0)   # error_if_nonfinite=False, as the reference calls it
    ob.step()
    assert bool(torch.isnan(oa.grad_norm).all()) and bool(torch.isnan(ref_norm))
    for x, y in zip(a[:NOGRAD], b[:NOGRAD]):
        assert bool(torch.isnan(x).all()) and bool(torch.isnan(y).all())
    assert not bool(torch.isnan(a[NOGRAD]).any())


# ---- 6. the models -------------------------------------------------------------------------------------------------------------------------

def _sr_model(fused_step_tail):
    from basicsr.models import build_model
    from dcpt_amd.keyed_init import keyed_input, keyed_state_dict
    from oracle import nafnet_oracle as O
    from tests.test_gpu_dcpt_step import TINY

    train = dict(pixel_opt=dict(type="L1Loss", loss_weight=1.0, reduction="mean"), optim_g=dict(type="AdamW", lr=1e-3, fused=True), ema_decay=0.9)
    if fused_step_tail:
        train["fused_step_tail"] = True
    m = build_model(dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True, grad_clip=GRAD_CLIP,
                         network_g=dict(type="NAFNetBaseline", **TINY), path=dict(), train=train))
    m.net_g.load_state_dict(keyed_state_dict(O.nafnet_param_shapes(**TINY), seed=0), strict=True)
    m.model_ema(0)
    m.feed_data({"lq": keyed_input("dcpt.lq", (2, 3, 32, 32)), "gt": keyed_input("dcpt.gt", (2, 3, 32, 32))})
    return m


def _dcdist_model(fused_step_tail):
    from dcpt_amd.keyed_init import keyed_input
    from tests.test_gpu_dcpt_step import _dist_model

    train = dict(pixel_opt=dict(type="L1Loss", loss_weight=1.0, reduction="mean"), classify_opt=dict(type="CrossEntropyLoss", loss_weight=1.0),
                 optim_g=dict(type="AdamW", lr=1e-3, fused=True), ema_decay=0.9)
    if fused_step_tail:
        train["fused_step_tail"] = True
    m = _dist_model(grad_clip=GRAD_CLIP, train=train)
    m.feed_data({"lq": keyed_input("dist.lq", (2, 3, 32, 32)), "gt": keyed_input("dist.gt", (2, 3, 32, 32)), "dataset_idx": torch.tensor([4, 1])})
    return m


def _after_one_step(m):
    m.optimize_parameters(1)
    out = {"net_g." + k: v.detach().clone() for k, v in m.net_g.named_parameters()}
    out.update({"net_g_ema." + k: v.detach().clone() for k, v in m.net_g_ema.named_parameters()})
    out.update({"exp_avg." + k: m.optimizer_g.state[v]["exp_avg"].clone() for k, v in m.net_g.named_parameters() if v in m.optimizer_g.state})
    return out


@pytest.mark.parametrize("build", [_sr_model, _dcdist_model], ids=["SRModel", "DCDistModel"])
def test_models_take_the_same_step_with_the_key_on(build, monkeypatch):
    from dcpt_amd.optim import FusedAdamW

    off1, off2 = _after_one_step(build(False)), _after_one_step(build(False))
    m = build(True)
    assert isinstance(m.optimizer_g, FusedAdamW) and m.fused_step_tail is True
    foreach = []
    real = torch._foreach_mul_
    monkeypatch.setattr(torch, "_foreach_mul_", lambda *a, **k: (foreach.append(1), real(*a, **k))[1])
    with kernel_trace() as t:
        on = _after_one_step(m)
    t.assert_ran("grad_norm.sumsq", "grad_norm.finish", "adamw.clip_ema")
    assert foreach == [], "the EMA copies ride in the AdamW kernel: no foreach pass"
    norm = float(m.optimizer_g.grad_norm)
    assert norm > 2 * GRAD_CLIP, norm   # grad_clip bites
    assert off1.keys() == on.keys() and any(k.startswith("exp_avg.") for k in on)
    for k in on:
        run_to_run = float((off1[k] - off2[k]).abs().max())
        diff = (on[k] - off1[k]).abs()
        if k.startswith("exp_avg."):   # test_gpu_optim.py's tolerance for the first moment
            allowed = 2 * run_to_run + 2e-6 * off1[k].abs() + 2e-7 * float(off1[k].abs().max())
        else:                          # test_gpu_optim.py:47, parameters
            allowed = 2 * run_to_run + 4e-6 * off1[k].abs() + 2e-7
        assert bool((diff <= allowed).all()), (k, float(diff.max()), run_to_run)
        if k.startswith("exp_avg.") and float(off1[k].abs().max()) > 0:   # a dropped coefficient would leave it 1 / coef times larger
            assert float(on[k].abs().max()) <= 1.001 * float(off1[k].abs().max())
