"""CPU: the yardstick of the LDL artifact weights (tests/ldl_restatement.py: its closed-form gradient against float64 autograd of its own
pad / unfold / torch.std expression, zero-variance windows included) and the public surface that needs no device: the workspace query and
the refusals of dcpt_ldl_weight_*, dcpt_amd.functional.ldl_weight on CPU tensors, basicsr.losses.loss_util.get_refined_artifact_map's
refusals, and SRModel's check of ``ldl_opt`` / ``ldl_std``.

The gradient bound is the one the GPU test uses, |g - T| <= 2^-23 |T| + 1e-9 max|T|; the closed form sits 10^5 and more below it
(printed per shape)."""
import inspect

import pytest
import torch

import ldl_restatement as R
from dcpt_amd.keyed_init import keyed_input
from tests import test_plumbing_cpu as TP   # registers the CPU stand-in arch ``_TestConvArch``

SHAPES = [(1, 1, 4, 4), (1, 3, 6, 7), (2, 3, 16, 32), (1, 3, 17, 33), (2, 3, 40, 75), (3, 1, 5, 50), (1, 1, 50, 4)]


def _inputs(tag, shape):
    gt = keyed_input(f"ldlcpu.{tag}.gt", shape)
    out = gt + keyed_input(f"ldlcpu.{tag}.n", shape, lo=-0.08, hi=0.08)
    gw = keyed_input(f"ldlcpu.{tag}.gw", shape, lo=-1.0, hi=1.0)
    return gt.double(), out.double(), gw.double()


def _autograd(gt, out, gw):
    leaf = out.clone().requires_grad_(True)
    w = R.artifact_map(gt, leaf)
    (w * gw).sum().backward()
    return w.detach(), leaf.grad


def _ratio(g, T):
    bound = 2.0 ** -23 * T.abs() + 1e-9 * float(T.abs().max())
    return float(((g - T).abs() / bound).max())


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_closed_form_gradient_matches_autograd(shape):
    gt, out, gw = _inputs(shape, shape)
    w, T = _autograd(gt, out, gw)
    g = R.weight_grad_closed_form(gt, out, gw)
    ratio = _ratio(g, T)
    print(f"closed form vs autograd {shape}: max|T| {float(T.abs().max()):.3e} worst ratio to the bound {ratio:.3e}")
    assert float(T.abs().max()) > 1e-4 and float(w.min()) > 0 and float(w.max()) < 1 and (gw < 0).any() and (gw > 0).any()
    assert ratio <= 1.0


def test_zero_variance_windows_give_a_finite_gradient_equal_to_the_masked_closed_form():
    """out == gt on the left half: every window inside it has u == 0 exactly.  torch's std backward masks those windows, the closed form
    masks them by ``Gv = 0 where u == 0``: both finite, both the same, and exactly 0 where no window with u > 0 reaches"""
    shape = (1, 3, 24, 40)
    gt, out, gw = _inputs("zero", shape)
    out[..., :20] = gt[..., :20]
    u = R.local_std((gt - out).abs())
    assert int((u == 0).sum()) == 3 * 24 * 17 and float(u[..., 17:].min()) > 0
    w, T = _autograd(gt, out, gw)
    g = R.weight_grad_closed_form(gt, out, gw)
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(T).all()) and bool(torch.isfinite(g).all())
    ratio = _ratio(g, T)
    print(f"zero-variance half {shape}: max|T| {float(T.abs().max()):.3e} worst ratio to the bound {ratio:.3e}")
    assert ratio <= 1.0
    assert float(T[..., :20].abs().max()) == 0.0 and float(g[..., :20].abs().max()) == 0.0   # (sign(0) = 0 wherever out == gt)


def test_box_transpose_is_the_transpose_of_pad_then_box():
    """<box(pad(x)), y> == <x, T(y)> for the restatement's T, at sizes where the two folds of an axis overlap and where they do not"""
    import torch.nn.functional as F

    for shape in [(1, 1, 4, 4), (1, 2, 6, 5), (2, 1, 9, 12)]:
        x, y = keyed_input(f"ldlcpu.tx{shape}", shape).double(), keyed_input(f"ldlcpu.ty{shape}", shape).double()
        fx = F.avg_pool2d(F.pad(x, [3, 3, 3, 3], mode="reflect"), 7, stride=1) * 49
        lhs, rhs = float((fx * y).sum()), float((x * R.box_transpose(y)).sum())
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_workspace_queries_need_no_device():
    from dcpt_amd import _lib

    q = _lib.load().dcpt_ldl_weight_ws_bytes
    for B, C, H, W in SHAPES + [(32, 3, 256, 256)]:
        f, b = q(B, C, H, W, 0), q(B, C, H, W, 1)
        n = B * C * H * W
        assert f >= 2 * 8 * n and b >= f + 2 * 8 * n, (B, C, H, W, f, b)   # two fp64 planes forward, two more backward
    assert q(32, 3, 256, 256, 1) < 4 * 8 * 32 * 3 * 256 * 256 + (1 << 20)
    for bad in [(0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 3, 16), (1, 3, 16, 3), (1, 1, 1, 1), (65536, 1, 4, 4), (256, 257, 4, 4)]:
        assert q(*bad, 0) == 0 and q(*bad, 1) == 0, bad
    assert q(65535, 1, 4, 4, 1) > 0


def test_entry_points_refuse_bad_arguments_without_a_device():
    """every check comes before the first launch: each refusal is reported, with its text, on a machine with no GPU"""
    from kernel_trace import kernel_trace

    from dcpt_amd import _lib

    lib = _lib.load()
    fwd, bwd, big = lib.dcpt_ldl_weight_fwd, lib.dcpt_ldl_weight_bwd, 1 << 30
    with kernel_trace() as t:
        for args in [(None, 8, 8, 8, big), (8, None, 8, 8, big), (8, 8, None, 8, big)]:
            assert fwd(*args, 1, 3, 16, 16, None) != 0 and b"null" in lib.dcpt_last_error()
        for args in [(None, 8, 8, 8, 8, big), (8, None, 8, 8, 8, big), (8, 8, None, 8, 8, big), (8, 8, 8, None, 8, big)]:
            assert bwd(*args, 1, 3, 16, 16, None) != 0 and b"null" in lib.dcpt_last_error()
        for dims, text in [((1, 3, 3, 16), b"H >= 4 and W >= 4"), ((1, 3, 16, 3), b"H >= 4 and W >= 4"), ((1, 1, 1, 1), b"B * C * H * W >= 2"),
                           ((65536, 1, 4, 4), b"B * C above 65535"), ((0, 3, 16, 16), b"bad shape")]:
            assert fwd(8, 8, 8, 8, big, *dims, None) != 0 and text in lib.dcpt_last_error(), (dims, lib.dcpt_last_error())
            assert bwd(8, 8, 8, 8, 8, big, *dims, None) != 0 and text in lib.dcpt_last_error(), (dims, lib.dcpt_last_error())
        nf, nb = lib.dcpt_ldl_weight_ws_bytes(1, 3, 16, 16, 0), lib.dcpt_ldl_weight_ws_bytes(1, 3, 16, 16, 1)
        assert fwd(8, 8, 8, 8, nf - 1, 1, 3, 16, 16, None) == 2 and b"workspace too small" in lib.dcpt_last_error()
        assert fwd(8, 8, 8, None, big, 1, 3, 16, 16, None) == 2 and b"workspace too small" in lib.dcpt_last_error()
        assert bwd(8, 8, 8, 8, 8, nb - 1, 1, 3, 16, 16, None) == 2 and b"workspace too small" in lib.dcpt_last_error()
        assert bwd(8, 8, 8, 8, 8, nf, 1, 3, 16, 16, None) == 2 and b"workspace too small" in lib.dcpt_last_error()   # the forward's size
        assert bwd(8, 8, 8, 8, None, big, 1, 3, 16, 16, None) == 2 and b"workspace too small" in lib.dcpt_last_error()
    assert t.counts == {}, t.counts
    assert lib.dcpt_abi_version() == 16


def test_cpu_tensors_raise_and_the_target_takes_no_gradient():
    from basicsr.losses.loss_util import get_refined_artifact_map
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    gt, out = keyed_input("ldlcpu.cpu.gt", (1, 3, 8, 8)), keyed_input("ldlcpu.cpu.out", (1, 3, 8, 8))
    for call in (lambda: DF.ldl_weight(gt, out), lambda: get_refined_artifact_map(gt, out, std=True)):
        with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
            call()
    with pytest.raises(_lib.DcptHipError):
        DF.ldl_weight(gt.numpy(), out.numpy())


def test_get_refined_artifact_map_keeps_the_signature_and_refuses_what_is_not_built():
    import basicsr.losses.loss_util as LU
    from basicsr.losses.loss_util import get_refined_artifact_map

    sig = [(p.name, p.default) for p in inspect.signature(get_refined_artifact_map).parameters.values()]
    E = inspect.Parameter.empty
    assert sig == [("img_gt", E), ("img_output", E), ("img_ema", None), ("ksize", 7), ("std", False)]
    assert "get_refined_artifact_map" in LU.__all__
    gt, out = keyed_input("ldlcpu.sig.gt", (1, 3, 8, 8)), keyed_input("ldlcpu.sig.out", (1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="img_ema that SRModel never passes"):
        get_refined_artifact_map(gt, out)
    with pytest.raises(NotImplementedError, match="img_ema that SRModel never passes"):
        get_refined_artifact_map(gt, out, std=False)
    with pytest.raises(NotImplementedError, match="ksize=5"):
        get_refined_artifact_map(gt, out, ksize=5, std=True)


def _train_opt(**train):
    opt = TP._opt(model_type="SRModel", is_train=True)
    opt["train"] = dict(optim_g=dict(type="Adam", lr=1e-3), **train)
    return opt


def test_srmodel_checks_the_ldl_options_at_set_up():
    from basicsr.models import build_model

    l1 = dict(type="L1Loss", loss_weight=1.0, reduction="mean")
    ldl = dict(type="L1Loss", loss_weight=1.0, reduction="none")
    for extra in ({}, {"ldl_std": False}, {"ldl_std": None}):
        with pytest.raises(ValueError, match="ldl_std: true"):
            build_model(_train_opt(pixel_opt=dict(l1), ldl_opt=dict(ldl), **extra))
    with pytest.raises(ValueError, match="Both pixel and perceptual losses are None"):
        build_model(_train_opt())
    m = build_model(_train_opt(pixel_opt=dict(l1), ldl_opt=dict(ldl), ldl_std=True))
    assert m.cri_pix is not None and m.cri_ldl is not None and m.cri_ldl.reduction == "none"
    m = build_model(_train_opt(ldl_opt=dict(ldl), ldl_std=True))   # the LDL term alone is a loss
    assert m.cri_pix is None and m.cri_ldl is not None
    m = build_model(_train_opt(pixel_opt=dict(l1)))
    assert m.cri_ldl is None
    # without ldl_opt a step on the CPU stand-in runs as before and logs l_pix alone
    g = torch.Generator().manual_seed(5)
    m.feed_data({"lq": torch.rand(2, 3, 16, 16, generator=g), "gt": torch.rand(2, 3, 16, 16, generator=g)})
    m.optimize_parameters(1)
    assert list(m.get_current_log()) == ["l_pix"]
