"""GPU: the LDL artifact weights on the fused fp64 kernels (dcpt_amd/csrc/ldl.hip through DF.ldl_weight,
basicsr.losses.loss_util.get_refined_artifact_map and SRModel's ``train.ldl_opt``) against tests/ldl_restatement.py, the kernel-blind
float64 restatement on the CPU.

Inputs: ``gt`` in [0, 1], ``out = gt + noise`` with the noise in +-0.08 and never clamped, so every 7 x 7 window has a variance far from
zero; the upstream gradient Gw is a keyed map with both signs.  The reference gradient is float64 autograd of the restatement on a float64
leaf holding the fp32 values.

Bounds (set by the arithmetic, not tuned):
* w, every element: |w - w64| <= 2^-24 + 1e-12 -- one fp32 ulp below 1 for the single rounding, plus a cap on what another order of the
  fp64 sums can move (two CPU orders differ by 5e-15).
* Gradient, every element: |g - T| <= 2^-23 |T| + 1e-9 max|T|, and max|T| > 1e-4 so that the case is not vacuous.
* SRModel step: ``l_ldl`` within the w bound times the mean of the element-wise loss the weights multiply.  Parameter gradients: the test
  this one is modelled on (test_training_step_with_ssim_loss) carries no numeric tolerance -- finite gradients, most parameters moved -- and
  both are asserted here; on top of that each parameter tensor agrees within 2e-4 of its largest element, the scale-relative bound of the
  fp32 step parity tests (tests/test_gpu_parity.py).  The reasoning: both steps run the same fp32 backward kernels, on output gradients
  that differ by at most 2^-22 of each element (one rounding each side); what is left is the fp32 rounding of those kernels' own sums.

Every case prints its worst figure as a ratio to its bound before it asserts.  Measured on the MI355X: every w at 0.48-0.50 of its bound
(the fp32 rounding alone), the worst gradient element at 0.40-0.48 of its bound over the seven shapes (max|T| 37-130) and at 0.48 in the
zero-variance case (max|T| 12.5); the SRModel step's l_ldl and every parameter gradient equal to the restated step's bit for bit, for both
reductions."""
import math

import pytest
import torch

import ldl_restatement as R
from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
W_TOL = 2.0 ** -24 + 1e-12
TH, TW = 16, 32   # DF.METRIC_TILE: pixels per workgroup of the tile and gather kernels
# (B, C, H, W) -- and what the shape is there for
CASES = {
    "all_halo": (1, 1, 4, 4),          # every window is all halo; the folds from both sides overlap
    "overlap_odd": (1, 3, 6, 7),       # overlapping folds on both axes; odd sizes
    "one_tile": (2, 3, TH, TW),        # exactly one tile; the global sums cross images and channels
    "past_tile": (1, 3, TH + 1, TW + 1),   # one pixel past the tile on each axis
    "ragged": (2, 3, 40, 75),          # several ragged tiles
    "thin_rows": (3, 1, 5, 50),
    "thin_cols": (1, 1, 50, 4),
}
ZERO_HALF = (1, 3, 24, 40)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    _lib.load()
    assert DF.METRIC_TILE == (TH, TW)
    return torch.device("cuda:0")


def _inputs(name, kind="noisy"):
    shape = CASES[name] if name in CASES else name
    gt = keyed_input(f"gpuldl.{name}.gt", shape)
    out = gt + keyed_input(f"gpuldl.{name}.n", shape, lo=-0.08, hi=0.08)
    if kind == "zero_half":
        out[..., : shape[3] // 2] = gt[..., : shape[3] // 2]
    elif kind == "same":
        out = gt.clone()
    return gt, out, keyed_input(f"gpuldl.{name}.gw", shape, lo=-1.0, hi=1.0)


_REF = {}


def _reference(name, kind="noisy"):
    """(w, gradient of sum(Gw w) with respect to out) of the restatement in float64: computed once per case and shared"""
    if (name, kind) not in _REF:
        gt, out, gw = _inputs(name, kind)
        leaf = out.double().requires_grad_(True)
        w = R.artifact_map(gt.double(), leaf)
        (w * gw.double()).sum().backward()
        _REF[name, kind] = (w.detach(), leaf.grad)
    return _REF[name, kind]


def _run(name, kind, dev):
    from dcpt_amd import functional as DF

    gt, out, gw = _inputs(name, kind)
    o = out.to(dev).requires_grad_(True)
    w = DF.ldl_weight(gt.to(dev), o)
    (w * gw.to(dev)).sum().backward()
    return w.detach().cpu(), o.grad.cpu()


def _w_ratio(w, T):
    return float((w.double() - T).abs().max()) / W_TOL


def _grad_ratio(g, T):
    """the worst |g - T| as a ratio to the bound 2^-23 |T| + 1e-9 max|T|"""
    T = T.double()
    bound = 2.0 ** -23 * T.abs() + 1e-9 * float(T.abs().max())
    return float(((g.double() - T).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("name", list(CASES))
def test_weights_and_gradient_match_the_restatement(name, dev):
    shape = CASES[name]
    w, g = _run(name, "noisy", dev)
    Tw, Tg = _reference(name)
    assert w.dtype == torch.float32 and g.dtype == torch.float32 and tuple(w.shape) == shape and tuple(g.shape) == shape
    rw, rg = _w_ratio(w, Tw), _grad_ratio(g, Tg)
    print(f"ldl_weight {name} {shape}: w in [{float(Tw.min()):.4f}, {float(Tw.max()):.4f}] worst ratio to the bound {rw:.3f}; "
          f"gradient max|T| {float(Tg.abs().max()):.3e} worst ratio to the bound {rg:.3f}")
    assert float(Tg.abs().max()) > 1e-4
    assert rw <= 1.0
    assert rg <= 1.0


def test_zero_variance_windows(dev):
    """out == gt on the left half: the windows inside it have u == 0 exactly (the tile's pivot is then 0 and the shifted sums are sums of
    zeros), the weights there are the floor tanh((0 - m) / s), the gradient is masked as torch's std backward masks it and is bitwise 0
    wherever out == gt"""
    w, g = _run(ZERO_HALF, "zero_half", dev)
    Tw, Tg = _reference(ZERO_HALF, "zero_half")
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(Tg).all())
    rw, rg = _w_ratio(w, Tw), _grad_ratio(g, Tg)
    print(f"ldl_weight zero-variance half {ZERO_HALF}: w worst ratio {rw:.3f}; gradient max|T| {float(Tg.abs().max()):.3e} worst ratio {rg:.3f}")
    assert float(Tg.abs().max()) > 1e-4 and rw <= 1.0 and rg <= 1.0
    half = ZERO_HALF[3] // 2
    assert int(g[..., :half].contiguous().view(torch.int32).abs().max()) == 0 and float(Tg[..., :half].abs().max()) == 0.0
    assert len(torch.unique(w[..., : half - 3])) == 1   # one value wherever the whole window lies in the left half


def test_identical_images_give_nan_weights_as_the_reference_does(dev):
    """out == gt everywhere: u = 0, m = 0, s = 0 and z = 0 / 0, so the reference's expression is NaN everywhere, and so is ours.  It is
    arithmetic only; nothing but w receives a non-finite value that leaves the call (the guards behind w and the workspace hold)."""
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    shape = (2, 3, TH + 1, TW + 1)
    gt, out, _ = _inputs(shape, "same")
    assert bool(torch.isnan(R.artifact_map(gt.double(), out.double())).all())
    w = DF.ldl_weight(gt.to(dev), out.to(dev))
    assert bool(torch.isnan(w).all())
    n = math.prod(shape)
    nf = lib.dcpt_ldl_weight_ws_bytes(*shape, 0)
    with redzone() as rz:
        wbuf, ws = DF._workspace(dev, 4 * n), DF._workspace(dev, nf)
        DF._call(lib.dcpt_ldl_weight_fwd, (gt.to(dev), out.to(dev), wbuf, ws, nf), shape, dev)
    assert rz.count == 2 and bool(torch.isnan(wbuf.view(torch.float32)).all())


def test_two_runs_give_identical_bits(dev):
    w1, g1 = _run("ragged", "noisy", dev)
    w2, g2 = _run("ragged", "noisy", dev)
    assert torch.equal(w1.view(torch.int32), w2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))


def test_noncontiguous_inputs_and_argument_checks(dev):
    from basicsr.losses.loss_util import get_refined_artifact_map
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    gt, out, gw = (t.to(dev) for t in _inputs("past_tile"))
    w = DF.ldl_weight(gt, out)
    w2 = get_refined_artifact_map(gt.contiguous(memory_format=torch.channels_last), torch.cat([out, out], 3)[..., : out.shape[3]], std=True)
    assert torch.equal(w.view(torch.int32), w2.contiguous().view(torch.int32))
    with pytest.raises(NotImplementedError, match="detach the target"):
        DF.ldl_weight(gt.clone().requires_grad_(True), out)
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        DF.ldl_weight(gt, out.cpu())
    with pytest.raises(_lib.DcptHipError, match="fp32"):
        DF.ldl_weight(gt.double(), out.double())
    with pytest.raises(ValueError):
        DF.ldl_weight(gt, out[..., :-1])
    with pytest.raises(_lib.DcptHipError, match="H >= 4 and W >= 4"):
        DF.ldl_weight(gt[..., :3], out[..., :3])


def test_launch_trace_names_the_ldl_kernels(dev):
    """a forward and backward pair runs the nine documented launches and nothing else of the library"""
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    gt, out, gw = (t.to(dev) for t in _inputs("ragged"))
    with kernel_trace() as t:
        o = out.requires_grad_(True)
        (DF.ldl_weight(gt, o) * gw).sum().backward()
    assert t.counts == {"ldl.tile": 1, "ldl.reduce": 3, "ldl.dev": 1, "ldl.w": 1, "ldl.gz": 1, "ldl.gv": 1, "ldl.gather": 1}, t.counts
    with kernel_trace() as t:   # without a gradient: the forward's five
        DF.ldl_weight(gt, out.detach())
    assert t.counts == {"ldl.tile": 1, "ldl.reduce": 2, "ldl.dev": 1, "ldl.w": 1}, t.counts


def test_stays_inside_its_buffers(dev):
    """the entry points on buffers of exactly the size they ask for, with guards behind w, dout and the workspace (all of them start as
    NaN patterns: nothing unwritten is read), on the ragged case; the bits are those of the autograd route"""
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    shape = CASES["ragged"]
    n = math.prod(shape)
    gt, out, gw = (t.to(dev) for t in _inputs("ragged"))
    o = out.clone().requires_grad_(True)
    w = DF.ldl_weight(gt, o)
    (w * gw).sum().backward()
    nf, nb = lib.dcpt_ldl_weight_ws_bytes(*shape, 0), lib.dcpt_ldl_weight_ws_bytes(*shape, 1)
    with redzone() as rz:
        w_f, ws_f = DF._workspace(dev, 4 * n), DF._workspace(dev, nf)   # the forward alone, on the forward's size
        DF._call(lib.dcpt_ldl_weight_fwd, (gt, out, w_f, ws_f, nf), shape, dev)
        w_b, dout, ws_b = DF._workspace(dev, 4 * n), DF._workspace(dev, 4 * n), DF._workspace(dev, nb)   # the pair, on the backward's size
        DF._call(lib.dcpt_ldl_weight_fwd, (gt, out, w_b, ws_b, nb), shape, dev)
        DF._call(lib.dcpt_ldl_weight_bwd, (gt, out, gw, dout, ws_b, nb), shape, dev)
    assert rz.count == 5
    for buf in (w_f, w_b):
        assert torch.equal(buf.view(torch.int32), w.detach().reshape(-1).view(torch.int32))
    assert torch.equal(dout.view(torch.int32), o.grad.reshape(-1).view(torch.int32))


def _step_model(ldl_opt):
    from basicsr.models import build_model
    from dcpt_amd.keyed_init import fill_module_

    tiny = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1])
    train = dict(pixel_opt=dict(type="L1Loss"), optim_g=dict(type="SGD", lr=0.05))
    if ldl_opt is not None:
        train.update(ldl_opt=ldl_opt, ldl_std=True)
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
               network_g=dict(type="NAFNetBaseline", window_size=16, **tiny), path=dict(pretrain_network_g=None), train=train)
    m = build_model(opt)
    fill_module_(m.net_g)
    return m


@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_training_step_with_the_ldl_term(reduction, dev, monkeypatch):
    """one SRModel.optimize_parameters step of a tiny NAFNetBaseline under pixel_opt L1Loss + ldl_opt L1Loss: against the same step with
    the weights computed by the restatement's torch expression on the device (float64, rounded once to fp32, autograd through it)"""
    import basicsr.models.sr_model as SM
    from kernel_trace import kernel_trace

    gt, _, _ = _inputs((2, 3, 32, 32))
    lq = keyed_input("gpuldl.step.lq", (2, 3, 32, 32))
    ldl_opt = dict(type="L1Loss", loss_weight=1.0, reduction=reduction)

    a = _step_model(ldl_opt)
    before = [p.detach().clone() for p in a.net_g.parameters()]
    a.feed_data({"lq": lq, "gt": gt})
    with kernel_trace() as t:
        a.optimize_parameters(1)
    assert t.families("ldl.") == {"ldl.tile": 1, "ldl.reduce": 3, "ldl.dev": 1, "ldl.w": 1, "ldl.gz": 1, "ldl.gv": 1, "ldl.gather": 1}
    log_a = a.get_current_log()

    b = _step_model(ldl_opt)
    monkeypatch.setattr(SM, "get_refined_artifact_map", lambda g, o, std: R.artifact_map(g.double(), o.double()).float())
    b.feed_data({"lq": lq, "gt": gt})
    with kernel_trace() as t:
        b.optimize_parameters(1)
    assert t.families("ldl.") == {}
    log_b = b.get_current_log()

    assert torch.equal(a.output.detach(), b.output.detach())   # the same network on the same input: the steps differ in the weights alone
    mag = float((a.output.detach() - a.gt).abs().double().mean())   # the mean of the element-wise L1 term (reduction none), its value (mean)
    d = abs(log_a["l_ldl"] - log_b["l_ldl"])
    print(f"SRModel step, ldl_opt reduction {reduction}: l_pix {log_a['l_pix']!r} l_ldl {log_a['l_ldl']!r} against {log_b['l_ldl']!r}: "
          f"|d| {d:.3e}, ratio to the bound {d / (W_TOL * mag):.3f}")
    assert list(log_a) == ["l_pix", "l_ldl"] and math.isfinite(log_a["l_ldl"]) and 0 < log_a["l_ldl"] < mag
    assert log_a["l_pix"] == log_b["l_pix"]
    assert d <= W_TOL * mag
    worst = 0.0
    for (k, p), q in zip(a.net_g.named_parameters(), b.net_g.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
        worst = max(worst, float((p.grad - q.grad).abs().max()) / float(q.grad.abs().max()))
    print(f"SRModel step, ldl_opt reduction {reduction}: worst scale-relative parameter-gradient difference {worst:.3e} (bound 2e-4)")
    assert worst <= 2e-4
    assert sum(int(not torch.equal(x, y.detach())) for x, y in zip(before, a.net_g.parameters())) > len(before) // 2
    # the LDL term is in the gradients: the step without it has other ones
    c = _step_model(None)
    c.feed_data({"lq": lq, "gt": gt})
    c.optimize_parameters(1)
    assert any(not torch.equal(p.grad, q.grad) for p, q in zip(a.net_g.parameters(), c.net_g.parameters()))


def test_a_step_without_ldl_opt_launches_no_ldl_kernel(dev):
    from kernel_trace import kernel_trace

    m = _step_model(None)
    assert m.cri_ldl is None
    m.feed_data({"lq": keyed_input("gpuldl.step.lq", (2, 3, 32, 32)), "gt": _inputs((2, 3, 32, 32))[0]})
    with kernel_trace() as t:
        m.optimize_parameters(1)
    assert t.counts and t.families("ldl.") == {} and list(m.get_current_log()) == ["l_pix"]
