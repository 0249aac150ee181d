"""CPU: the public surface of the SSIM losses (registries, constructor defaults, no CPU fallback, the workspace query of
dcpt_ssim_loss_*), and the yardstick itself: tests/ssim_restatement.py's closed-form gradient against autograd, its Gaussian against
basicsr.metrics._gauss_kernel, and the documented order of the fp32 luma against the reference's matmul form."""
import inspect

import numpy as np
import pytest
import torch

import ssim_restatement as R
from dcpt_amd.keyed_init import keyed_input

METRIC_Y = 1


def _pair(tag, shape, noise=0.08):
    a = keyed_input(f"{tag}.a", shape)
    b = (a + keyed_input(f"{tag}.n", shape, lo=-noise, hi=noise)).clamp(0, 1)
    return a, b


def test_losses_and_metric_are_registered():
    import basicsr.losses as L
    import basicsr.metrics as M
    from basicsr.utils.registry import LOSS_REGISTRY, METRIC_REGISTRY

    for name in ("SmoothL1Loss", "HuberLoss", "SSIMLoss", "SSIMMSELoss"):
        assert LOSS_REGISTRY.get(name) is getattr(L, name) and name in L.__all__
        assert isinstance(L.build_loss(dict(type=name)), getattr(L, name))
    assert METRIC_REGISTRY.get("calculate_ssim_pt") is M.calculate_ssim_pt and "calculate_ssim_pt" in M.__all__


def test_constructor_and_function_defaults_are_the_references():
    """basic_loss.py:89-232 and psnr_ssim.py:436-443: names, order and defaults of the arguments"""
    import basicsr.losses as L
    from basicsr.metrics import calculate_ssim_pt

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.name != "self"]

    E = inspect.Parameter.empty
    assert sig(L.SmoothL1Loss.__init__) == [("loss_weight", 1.0), ("reduction", "mean")]
    assert sig(L.HuberLoss.__init__) == [("loss_weight", 1.0), ("delta", 0.01), ("reduction", "mean")]
    both = [("ssim_weight", 0.1), ("mse_weight", 1.0), ("crop_border", 0), ("reduction", "mean"), ("test_y_channel", False)]
    assert sig(L.SSIMLoss.__init__) == both and sig(L.SSIMMSELoss.__init__) == both
    assert sig(calculate_ssim_pt) == [("img", E), ("img2", E), ("crop_border", E), ("test_y_channel", False), ("image_range", 255), ("kwargs", E)]
    assert sig(L.SSIMLoss.forward)[:3] == [("pred", E), ("target", E), ("weight", None)]
    assert [n for n, _ in sig(L.SSIMMSELoss.forward)] == ["pred", "target", "kwargs"]
    for cls in (L.SmoothL1Loss, L.HuberLoss):
        with pytest.raises(ValueError):
            cls(reduction="median")


def test_huber_and_smooth_l1_are_the_references_expressions():
    """plain torch on any device: HuberLoss is the reference's huber_loss (delta 0.01, not divided by delta) under its weight rule,
    SmoothL1Loss is F.smooth_l1_loss and ignores the weight"""
    import basicsr.losses as L

    a, b = _pair("ssimcpu.huber", (2, 3, 9, 7), noise=0.03)
    w3, w1 = keyed_input("ssimcpu.w3", (2, 3, 9, 7)), keyed_input("ssimcpu.w1", (2, 1, 9, 7))
    d = (a - b).abs().double()
    want = torch.where(d <= 0.01, 0.5 * d * d, 0.5 * 0.01 ** 2 + (d - 0.01))
    assert float((d <= 0.01).double().mean()) not in (0.0, 1.0)   # both branches occur
    assert abs(float(L.HuberLoss()(a, b)) - float(want.mean())) <= 1e-7 * float(want.mean())
    assert abs(float(L.HuberLoss(loss_weight=2.0, reduction="sum")(a, b, w3)) - 2 * float((want * w3).sum())) <= 1e-6 * float(want.sum())
    assert abs(float(L.HuberLoss()(a, b, w3)) - float((want * w3).sum() / w3.double().sum())) <= 1e-7
    assert abs(float(L.HuberLoss()(a, b, w1)) - float((want * w1).sum() / (w1.double().sum() * 3))) <= 1e-7
    assert tuple(L.HuberLoss(reduction="none")(a, b).shape) == (2, 3, 9, 7)
    assert torch.equal(L.SmoothL1Loss(loss_weight=3.0)(a, b, w3), 3.0 * torch.nn.functional.smooth_l1_loss(a, b))
    # the restatement's own forms of the same rule
    assert abs(float(R.huber_loss(a, b, w1)) - float((want * w1).sum() / (w1.double().sum() * 3))) <= 1e-9


def test_cpu_tensors_raise():
    import basicsr.losses as L
    from basicsr.metrics import calculate_ssim_pt
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    a, b = _pair("ssimcpu.cpu", (1, 3, 12, 12))
    for call in (lambda: DF.ssim_pt(a, b), lambda: calculate_ssim_pt(a, b, 0), lambda: L.SSIMLoss()(a, b), lambda: L.SSIMMSELoss()(a, b)):
        with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
            call()


def test_workspace_query_refuses_and_caps():
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    q = _lib.load().dcpt_ssim_loss_ws_bytes
    assert q(2, 3, 40, 75, 3, 0, 0) > 0 and q(2, 3, 40, 75, 3, METRIC_Y, 1) > 0 and q(1, 1, 11, 11, 0, 0, 1) > 0
    for bad in [(0, 3, 40, 40, 0, 0), (2, 2, 40, 40, 0, 0), (2, 4, 40, 40, 0, 0), (2, 3, 40, 40, -1, 0), (2, 3, 40, 40, 0, 2), (2, 3, 40, 40, 0, 4),
                (2, 3, 40, 40, 0, 8), (2, 3, 40, 40, 15, 0), (2, 3, 10, 40, 0, 0), (2, 3, 40, 10, 0, 0), (2, 3, 16, 16, 3, 0), (21846, 3, 11, 11, 0, 0),
                (2, 3, 0, 40, 0, 0)]:
        for backward in (0, 1):
            assert q(*bad, backward) == 0, bad
    assert q(21845, 3, 11, 11, 0, 0, 1) > 0   # B * C = 65535
    # the planes: 24 bytes per map position; the whole batch while it fits the cap, then whole images, never less than one
    cap = DF.ssim_plane_cap()
    assert cap == 64 << 20
    planes = lambda B, C, H, W: q(B, C, H, W, 0, 0, 1) - q(B, C, H, W, 0, 0, 0)   # noqa: E731
    per = 3 * 24 * 246 * 246
    assert per <= planes(1, 3, 256, 256) < per + 256
    assert 15 * per <= planes(32, 3, 256, 256) < 15 * per + 256 and 16 * per > cap   # 15 images of 4.36 MB under 64 MiB
    big = 3 * 24 * 2038 * 2038   # one image above the cap
    assert big > cap and big <= planes(4, 3, 2048, 2048) < big + 256
    assert planes(2, 3, 256, 256) >= 2 * per and planes(2, 3, 256, 256) < 2 * per + 256
    luma = q(2, 3, 256, 256, 0, METRIC_Y, 1) - q(2, 3, 256, 256, 0, METRIC_Y, 0)   # one map per image
    assert 2 * 24 * 246 * 246 <= luma < 2 * 24 * 246 * 246 + 256
    try:   # the test knob: the same query under a smaller cap
        assert DF.ssim_plane_cap(2 * per + 5) == 2 * per + 5
        assert 2 * per <= planes(5, 3, 256, 256) < 2 * per + 256
    finally:
        DF.ssim_plane_cap(cap)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """every check comes before the first launch: null pointers and refused shapes are reported on a machine with no GPU"""
    from dcpt_amd import _lib

    lib = _lib.load()
    assert lib.dcpt_ssim_loss_fwd(None, None, None, None, 0, 1, 3, 16, 16, 0, 0, 1.0, None) != 0 and b"null" in lib.dcpt_last_error()
    assert lib.dcpt_ssim_loss_bwd(8, 8, None, 8, None, 0, 1, 3, 16, 16, 0, 0, 1.0, None) != 0 and b"null" in lib.dcpt_last_error()
    assert lib.dcpt_ssim_loss_fwd(8, 8, 8, 8, 1 << 20, 1, 3, 16, 16, 3, 0, 1.0, None) != 0 and b"at least 11 x 11" in lib.dcpt_last_error()
    assert lib.dcpt_ssim_loss_fwd(8, 8, 8, 8, 1 << 20, 1, 2, 16, 16, 0, 0, 1.0, None) != 0 and b"C must be 1 or 3" in lib.dcpt_last_error()
    assert lib.dcpt_ssim_loss_bwd(8, 8, 8, 8, 8, 1 << 20, 1, 3, 16, 16, 0, 2, 1.0, None) != 0 and b"unknown flag" in lib.dcpt_last_error()
    assert lib.dcpt_ssim_loss_bwd(8, 8, 8, 8, 8, 1 << 20, 1, 3, 16, 16, 0, 0, 0.0, None) != 0 and b"image_range" in lib.dcpt_last_error()
    assert lib.dcpt_ssim_loss_fwd(8, 8, 8, 8, 8, 1, 3, 16, 16, 0, 0, 1.0, None) == 2 and b"workspace too small" in lib.dcpt_last_error()
    assert lib.dcpt_ssim_loss_bwd(8, 8, 8, 8, None, 1 << 20, 1, 3, 16, 16, 0, 0, 1.0, None) == 2 and b"workspace too small" in lib.dcpt_last_error()


def test_restatement_gaussian_is_the_projects():
    from basicsr.metrics import _gauss_kernel

    g = R.gauss().numpy()
    assert g.dtype == np.float64 and np.array_equal(g, _gauss_kernel()) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])


@pytest.mark.parametrize("shape", [(2, 3, 11, 11), (1, 1, 12, 29), (2, 3, 27, 40)])
def test_closed_form_gradient_matches_autograd(shape):
    """the formula the kernels implement (Pa, Pb, Pc and the transposed window, in separable passes) against autograd of the grouped-conv
    restatement: 1e-12 of the largest gradient"""
    a, b = _pair(f"ssimcpu.grad{shape}", shape, noise=0.1)
    x = a.double().requires_grad_(True)
    w = torch.linspace(0.5, 1.5, shape[0] * shape[1], dtype=torch.float64).view(shape[0], shape[1])
    (R.ssim_map(x, b.double()).sum((2, 3)) * w).sum().backward()
    got = R.ssim_grad_analytic(a.double(), b.double(), w)
    worst, scale = float((got - x.grad).abs().max()), float(x.grad.abs().max())
    print(f"closed form vs autograd {shape}: max|g| {scale:.3e} max diff {worst:.3e} relative {worst / scale:.3e}")
    assert scale > 0.1 and worst <= 1e-12 * scale
    # identical and zero images: the gradient vanishes
    for v in (a.double(), torch.zeros_like(a, dtype=torch.float64)):
        assert float(R.ssim_grad_analytic(v, v.clone(), w).abs().max()) <= 1e-9


@pytest.mark.parametrize("B, H, W, noise", [(2, 33, 21, 0.1), (1, 27, 43, 0.02), (2, 40, 75, 0.3)])
def test_documented_luma_order_against_the_matmul_form(B, H, W, noise):
    """SSIM on the luma in the documented order against SSIM on the reference's matmul luma: within 4 * 2^-24 * (sum |ds/dYx| + sum |ds/dYy|)
    + 1e-10 -- a first-order bound for luma values that differ by at most 4 fp32 half-ulps of values below 1.  Measured on the CPU this
    was written on: every luma value equal, difference 0."""
    p, t = _pair(f"ssimcpu.luma{H}x{W}", (B, 3, H, W), noise=noise)
    yp, yt = R.luma_ordered32(p), R.luma_ordered32(t)
    mp, mt = R.luma_matmul32(p), R.luma_matmul32(t)
    assert yp.dtype == mp.dtype == torch.float32
    Yp, Yt = yp.double().requires_grad_(True), yt.double().requires_grad_(True)
    s = R.ssim_map(Yp, Yt).mean([1, 2, 3])
    s_mm = R.ssim_map(mp.double(), mt.double()).mean([1, 2, 3])
    for b in range(B):
        gp, gt = torch.autograd.grad(s[b], [Yp, Yt], retain_graph=True)
        bound = 4 * 2.0 ** -24 * float(gp.abs().sum() + gt.abs().sum()) + 1e-10
        diff = abs(float(s_mm[b]) - float(s[b].detach()))
        print(f"luma {B}x{H}x{W} image {b}: ssim {float(s[b].detach())!r} |matmul - ordered| {diff:.3e} bound {bound:.3e} "
              f"equal luma values {float((yp == mp).float().mean()):.4f}")
        assert diff <= bound
    # the restatement's luma: the ordered fp32 value, the float64 gradient with the fp32 coefficients
    q = p.clone().requires_grad_(True)
    Y = R.luma(q)
    assert Y.dtype == torch.float64 and torch.equal(Y.detach(), yp.double())
    Y.sum().backward()
    c = torch.tensor(R.YCOEF, dtype=torch.float32).double() / 255.0
    assert torch.equal(q.grad, c.float().view(1, 3, 1, 1).expand_as(q))
