"""CPU: the host forms of the reference's remaining metrics -- ``calculate_msssim``, ``calculate_ssim_matlab``, ``calculate_nrmse``,
``calculate_psnr_pt`` (basicsr/metrics/__init__.py; reference basicsr/metrics/psnr_ssim.py:334-432, :201-330, :563-612, :79-110) -- against
independently written scipy / torch forms, their quirks pinned by construction, and the plumbing around them.

Tolerances (the derivation of tests/test_gpu_metrics.py's header): the host forms run two 1-D passes, the scipy forms one 2-D window, so
only the summation order differs -- 1e-10 absolute on every per-level SSIM / CS mean and on ``calculate_ssim_matlab``.  The final MS-SSIM
value is a product of powers of means x_k >= 0.5: its relative error is at most sum_k w_k 1e-10 / x_k <= 2e-10 sum_k w_k, held to 1e-9.
NRMSE and the box blur of quantised values are exact on both sides (``==``)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy import ndimage

from dcpt_amd.keyed_init import keyed_input

TOL = 1e-10
WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]


def _pair(tag, shape):
    """keyed uniform image + bounded noise clipped to [0, 1] (the recipe of tests/test_gpu_metrics.py::_pair)"""
    a = keyed_input(f"{tag}.a", shape).numpy()
    b = np.clip(a + keyed_input(f"{tag}.n", shape, lo=-0.08, hi=0.08).numpy(), 0, 1).astype(np.float32)
    return a, b


def _window():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    return np.outer(g / g.sum(), g / g.sum())


def _front(a, crop, rng):
    """(B, C, H, W) float in [0, 1] -> (B, H', W', C) float64 metric values, without luma (written directly, not through ``_images``)"""
    q = a.transpose(0, 2, 3, 1)
    if rng != 1:
        q = np.rint(q.astype(np.float32) * np.float32(rng))
    q = q.astype(np.float64)
    return q[:, crop:q.shape[1] - crop, crop:q.shape[2] - crop]


def _moments(x, y, mode):
    win = _window()
    f = lambda z: ndimage.correlate(z, win, mode=mode, cval=0.0)  # noqa: E731
    mx, my = f(x), f(y)
    return mx, my, f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my


def _scipy_ssim_cs(x, y, rng):
    """the published formula on the 'valid' positions: zero-padded 2-D correlation, the 5-pixel rim cut off"""
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    mx, my, sx, sy, sxy = (m[5:-5, 5:-5] for m in _moments(x, y, "constant"))
    cs = (2 * sxy + c2) / (sx + sy + c2)
    return (((2 * mx * my + c1) / (mx * mx + my * my + c1)) * cs).mean(), cs.mean()


def _scipy_blur(a):
    """the 2 x 2 box filter anchored at (0, 0), the edge replicated: per channel of (H, W, C)"""
    return np.stack([ndimage.correlate(a[..., j], np.full((2, 2), 0.25), mode="nearest", origin=-1) for j in range(a.shape[2])], axis=2)


def _scipy_msssim(a, b, crop, weights, rng):
    """returns (value, [[(ssim_k, cs_k)] per image])"""
    xs, ys = _front(a, crop, rng), _front(b, crop, rng)
    L, res, levels = len(weights), [], []
    for x, y in zip(xs, ys):
        sc = []
        for k in range(L):
            sc.append(_scipy_ssim_cs(x[..., k % x.shape[2]], y[..., k % x.shape[2]], rng))
            x, y = _scipy_blur(x), _scipy_blur(y)
        levels.append(sc)
        v = sc[L - 1][0] ** weights[L - 1]
        for k in range(L - 1):
            v *= sc[k][1] ** weights[k]
        res.append(v)
    return float(np.mean(res)), levels


def _scipy_matlab_channel(x, y, rng):
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    mx, my, sx, sy, sxy = _moments(x, y, "nearest")
    return (((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))).mean()


def _scipy_matlab(a, b, crop, rng):
    vals = []
    for x, y in zip(_front(a, crop, rng), _front(b, crop, rng)):
        per = [_scipy_matlab_channel(x[..., j], y[..., j], rng) for j in range(x.shape[2])]
        vals += per + [per[-1]]
    return float(np.mean(vals)), vals


# ---- 1. independent implementations -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, C, hw, crop, rng", [(2, 3, (46, 43), 3, 255), (1, 1, (31, 56), 3, 255), (2, 3, (17, 17), 3, 1), (1, 3, (11, 11), 0, 255)])
def test_msssim_matches_scipy_per_level(B, C, hw, crop, rng):
    import basicsr.metrics as M

    a, b = _pair(f"msm.ms.{hw[0]}x{hw[1]}", (B, C, *hw))
    want, levels = _scipy_msssim(a, b, crop, WEIGHTS, rng)
    worst = 0.0
    for i, (x, y) in enumerate(M._images(a, b, crop, "BCHW", False, rng)):
        bx, by = _front(a, crop, rng)[i], _front(b, crop, rng)[i]
        for k in range(5):
            if rng == 255:   # quantised: every blurred value is an integer over 4^k, exact on both sides
                assert np.array_equal(x, bx) and np.array_equal(y, by), (i, k)
            s, c = M._ssim_cs(x[..., k % C], y[..., k % C], rng)
            assert min(s, c) >= 0.5, (i, k, s, c)   # the premise of the 1e-9 bound on the product
            worst = max(worst, abs(s - levels[i][k][0]), abs(c - levels[i][k][1]))
            x, y, bx, by = M._box_blur(x), M._box_blur(y), _scipy_blur(bx), _scipy_blur(by)
    got = M.calculate_msssim(a, b, crop, image_range=rng)
    print(f"msssim {B}x{C}x{hw} crop {crop} range {rng}: host {got!r} scipy {want!r}; worst per-level mean difference {worst:.3e}")
    assert worst <= TOL
    assert abs(got - want) <= 1e-9
    for w in ([1.0], [0.5, 0.5], [0.125] * 8):
        assert abs(M.calculate_msssim(a, b, crop, weights=w, image_range=rng) - _scipy_msssim(a, b, crop, w, rng)[0]) <= 1e-9, w


def test_box_blur_is_the_anchored_filter_with_the_last_row_and_column_repeated():
    import basicsr.metrics as M

    a = np.arange(12, dtype=np.float64).reshape(3, 4, 1) ** 2
    out = M._box_blur(a)
    assert out.shape == a.shape and np.array_equal(out, _scipy_blur(a))
    assert out[0, 0, 0] == 0.25 * ((a[0, 0, 0] + a[0, 1, 0]) + (a[1, 0, 0] + a[1, 1, 0]))
    assert out[2, 3, 0] == a[2, 3, 0] and out[2, 0, 0] == 0.5 * (a[2, 0, 0] + a[2, 1, 0]) and out[0, 3, 0] == 0.5 * (a[0, 3, 0] + a[1, 3, 0])


@pytest.mark.parametrize("B, C, hw, crop, rng", [(2, 3, (46, 43), 3, 255), (1, 1, (9, 13), 2, 255), (2, 3, (7, 9), 3, 1), (1, 3, (1, 1), 0, 255),
                                                  (1, 1, (1, 7), 0, 1)])
def test_ssim_matlab_matches_scipy(B, C, hw, crop, rng):
    from basicsr.metrics import calculate_ssim_matlab

    a, b = _pair(f"msm.ml.{hw[0]}x{hw[1]}", (B, C, *hw))
    got, (want, _) = calculate_ssim_matlab(a, b, crop, image_range=rng), _scipy_matlab(a, b, crop, rng)
    print(f"ssim_matlab {B}x{C}x{hw} crop {crop} range {rng}: host {got!r} scipy {want!r} |d| {abs(got - want):.3e}")
    assert abs(got - want) <= TOL


@pytest.mark.parametrize("y", [False, True])
@pytest.mark.parametrize("rng", [255, 1])
def test_nrmse_is_the_formula(y, rng):
    import basicsr.metrics as M

    a, b = _pair("msm.nrmse", (3, 3, 21, 18))
    vals = []
    for x, z in M._images(a, b, 2, "BCHW", y, rng):   # (the front end itself is calculate_psnr's, pinned against the reference)
        vals.append(np.sqrt(np.mean((x - z) ** 2)) / (x.max() - x.min()))
    assert M.calculate_nrmse(a, b, 2, test_y_channel=y, image_range=rng) == float(np.mean(vals))
    if not y:
        x, z = _front(a, 2, rng), _front(b, 2, rng)
        direct = np.mean([np.sqrt(np.mean((x[i] - z[i]) ** 2)) / (x[i].max() - x[i].min()) for i in range(3)])
        assert M.calculate_nrmse(a, b, 2, image_range=rng) == float(direct)


# ---- 2. quirks pinned by construction ----------------------------------------------------------------------------------------------------
def test_msssim_channel_rotation():
    """evaluation k scores channel k mod C: with the default weights channel 1 enters at evaluations 1 and 4; with weights [1.0] only
    evaluation 0 on channel 0 counts"""
    from basicsr.metrics import calculate_msssim

    a, b = _pair("msm.rot", (1, 3, 30, 33))
    a2 = a.copy()
    a2[:, 1] = np.clip(a[:, 1] * 0.5 + 0.2, 0, 1)
    assert calculate_msssim(a2, b, 0) != calculate_msssim(a, b, 0)
    assert calculate_msssim(a2, b, 0, weights=[1.0]) == calculate_msssim(a, b, 0, weights=[1.0])
    a3 = a.copy()
    a3[:, 0] = np.clip(a[:, 0] * 0.5 + 0.2, 0, 1)
    assert calculate_msssim(a3, b, 0, weights=[1.0]) != calculate_msssim(a, b, 0, weights=[1.0])
    # weights [1.0]: the plain SSIM of channel 0
    from basicsr.metrics import calculate_ssim

    assert abs(calculate_msssim(a, b, 0, weights=[1.0]) - calculate_ssim(a[:, :1], b[:, :1], 0)) <= 1e-15


def test_ssim_matlab_counts_the_last_channel_twice():
    from basicsr.metrics import calculate_ssim_matlab

    a, _ = _pair("msm.twice", (1, 3, 20, 23))
    b = a.copy()
    b[:, 2] = np.clip(a[:, 2] + keyed_input("msm.twice.n", (1, 20, 23), lo=-0.1, hi=0.1).numpy(), 0, 1)
    C = 3
    s_last = calculate_ssim_matlab(a[:, 2:], b[:, 2:], 0)   # one channel: [s, s] -> s
    assert 0 < s_last < 0.999
    want = ((C - 1) * 1.0 + 2 * s_last) / (C + 1)   # [1, 1, s_last, s_last]
    assert abs(calculate_ssim_matlab(a, b, 0) - want) <= 1e-12
    # the first channel alone differing counts once
    b0 = a.copy()
    b0[:, 0] = b[:, 2]
    s0 = calculate_ssim_matlab(a[:, :1], b0[:, :1], 0)
    assert abs(calculate_ssim_matlab(a, b0, 0) - (s0 + 3.0) / 4) <= 1e-12


def test_nrmse_inf_and_identical_images():
    from basicsr.metrics import calculate_msssim, calculate_nrmse, calculate_ssim_matlab

    a, b = _pair("msm.inf", (3, 3, 24, 20))
    assert np.isfinite(calculate_nrmse(a, b, 0))
    b2 = b.copy()
    b2[1] = a[1]
    assert calculate_nrmse(a, b2, 0) == float("inf")
    for y in (False, True):
        assert abs(calculate_msssim(a, a.copy(), 2, test_y_channel=y) - 1.0) <= 1e-12
        assert abs(calculate_ssim_matlab(a, a.copy(), 2, test_y_channel=y) - 1.0) <= 1e-12
    with pytest.warns(RuntimeWarning):   # a constant first image divides by zero the way numpy does
        assert calculate_nrmse(np.full((1, 1, 8, 8), 0.5, np.float32), a[:1, :1, :8, :8], 0) == float("inf")


def test_existing_ssim_is_untouched_by_the_new_helper():
    import basicsr.metrics as M

    a, b = _pair("msm.same_ssim", (1, 1, 25, 27))
    x, y = next(M._images(a, b, 0, "BCHW", False, 255))
    assert M._ssim_cs(x[..., 0], y[..., 0])[0] == M._ssim(x[..., 0], y[..., 0])


# ---- 3. calculate_psnr_pt ---------------------------------------------------------------------------------------------------------------
def _psnr_pt_restated(img, img2, crop, y):
    if crop != 0:
        img, img2 = img[:, :, crop:-crop, crop:-crop], img2[:, :, crop:-crop, crop:-crop]
    if y and img.shape[1] == 3:
        from ssim_restatement import luma_matmul32

        img, img2 = luma_matmul32(img), luma_matmul32(img2)
    mse = torch.mean((img.to(torch.float64) - img2.to(torch.float64)) ** 2, dim=[1, 2, 3])
    return 10.0 * torch.log10(1.0 / (mse + 1e-12))


@pytest.mark.parametrize("crop", [0, 3])
@pytest.mark.parametrize("y", [False, True])
def test_psnr_pt(y, crop):
    from basicsr.metrics import calculate_psnr_pt

    a, b = (torch.from_numpy(t) for t in _pair("msm.pt", (3, 3, 19, 22)))
    got, want = calculate_psnr_pt(a, b, crop, test_y_channel=y), _psnr_pt_restated(a, b, crop, y)
    assert got.shape == (3,) and got.dtype == torch.float64
    if not y:
        assert torch.equal(got, want)
    else:
        assert torch.allclose(got, want, rtol=0, atol=1e-9)   # (the fp32 matmul's summation order is torch's own on both sides)
    assert torch.equal(calculate_psnr_pt(a[:, :1], b[:, :1], crop, test_y_channel=True), _psnr_pt_restated(a[:, :1], b[:, :1], crop, False))
    # no quantisation: far from calculate_psnr's value on an input that rounds to equal bytes
    tiny = calculate_psnr_pt(a, a + 1e-4, 0)
    assert bool(torch.isfinite(tiny).all()) and float(tiny.min()) > 70


def test_rgb2ycbcr_pt_equals_the_restatement():
    from ssim_restatement import luma_matmul32

    from basicsr.utils import rgb2ycbcr_pt

    a = torch.from_numpy(_pair("msm.ycc", (2, 3, 9, 11))[0])
    assert torch.equal(rgb2ycbcr_pt(a, y_only=True), luma_matmul32(a))
    full = rgb2ycbcr_pt(a)
    assert full.shape == a.shape and full.dtype == a.dtype
    assert torch.allclose(full[:, :1], luma_matmul32(a), rtol=0, atol=1e-6)
    w = torch.tensor([[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]], dtype=torch.float64)
    want = (torch.einsum("bchw,cd->bdhw", a.double(), w) + torch.tensor([16.0, 128.0, 128.0], dtype=torch.float64).view(1, 3, 1, 1)) / 255.0
    assert torch.allclose(full.double(), want, rtol=0, atol=1e-6)


# ---- 4. the deliberate fp64-for-fp32 deviation of calculate_ssim_matlab, measured ---------------------------------------------------------
def test_ssim_matlab_distance_to_the_reference_fp32_arithmetic():
    """Printed and recorded, not gated: ``calculate_ssim_matlab`` (float64) against the reference's arithmetic --
    ``.float()`` images through an fp32 ``Conv2d(1, 1, 11, padding=5, padding_mode="replicate")`` with the 2-D window -- restated in torch on
    the 40 x 37 pair.  Measured: 1.7e-7 with image_range 255 (values up to 255^2 in fp32 moments), 5.0e-8 with image_range 1."""
    from basicsr.metrics import calculate_ssim_matlab

    a, b = _pair("msm.fp32", (1, 3, 40, 37))
    win = torch.from_numpy(_window()).float().view(1, 1, 11, 11)
    for rng in (255, 1):
        c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
        conv = lambda t: F.conv2d(F.pad(t, (5, 5, 5, 5), mode="replicate"), win)  # noqa: E731
        vals = []
        for x, y in zip(_front(a, 0, rng), _front(b, 0, rng)):
            per = []
            for j in range(3):
                u, v = (torch.from_numpy(np.ascontiguousarray(t[..., j])).float()[None, None] for t in (x, y))
                mu1, mu2 = conv(u), conv(v)
                s1, s2, s12 = conv(u ** 2) - mu1 ** 2, conv(v ** 2) - mu2 ** 2, conv(u * v) - mu1 * mu2
                per.append((((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 ** 2 + mu2 ** 2 + c1) * (s1 + s2 + c2))).mean().item())
            vals += per + [per[-1]]
        d = abs(calculate_ssim_matlab(a, b, 0, image_range=rng) - float(np.mean(vals)))
        print(f"ssim_matlab float64 against the reference's fp32 Conv2d arithmetic, 1 x 3 x 40 x 37, image_range {rng}: |d| = {d:.3e}")
        assert np.isfinite(d)


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------------------
def test_registry_and_accumulator_defaults():
    import basicsr.metrics as M
    from basicsr.utils.registry import METRIC_REGISTRY

    names = ["calculate_msssim", "calculate_ssim_matlab", "calculate_nrmse", "calculate_psnr_pt", "calculate_msssim_device",
             "calculate_ssim_matlab_device", "calculate_nrmse_device"]
    for n in names:
        assert METRIC_REGISTRY.get(n) is getattr(M, n) and n in M.__all__
    a, b = _pair("msm.reg", (1, 3, 16, 16))
    assert M.calculate_metric(dict(img=a, img2=b), dict(type="calculate_nrmse", crop_border=1)) == M.calculate_nrmse(a, b, 1)
    assert M.MetricSums().result() == {"psnr": [], "ssim": []} and M.MetricSums().pending() == []
    assert list(M.MetricSums(msssim=True, nrmse=True).result()) == ["psnr", "ssim", "msssim", "nrmse"]
    with pytest.raises(ValueError):
        M.MetricSums(input_order="BHWC", msssim=True)


def test_abi_of_the_new_entry_points_without_a_gpu():
    """the workspace queries need no device and return 0 for refused arguments; each refusal is named before any launch"""
    from dcpt_amd import _lib

    lib = _lib.load()
    Y, R1 = 1, 4
    assert lib.dcpt_msssim_ws_bytes(2, 3, 40, 50, 3, Y, 5) > 0 and lib.dcpt_ssim_matlab_ws_bytes(2, 3, 1, 1, 0, R1) > 0
    assert lib.dcpt_imgrange_ws_bytes(2, 3, 40, 50, 3, 0) > 0
    # one tile per (image, level): 2 doubles each, rounded up to the allocator's 256 bytes
    assert lib.dcpt_msssim_ws_bytes(1, 3, 11, 11, 0, 0, 8) == 256 and lib.dcpt_msssim_ws_bytes(4, 3, 26, 42, 0, 0, 8) == 512
    assert lib.dcpt_msssim_ws_bytes(4, 3, 27, 42, 0, 0, 8) == 1024
    for args, words in [((1, 2, 40, 50, 0, 0, 5), b"C must be 1 or 3"), ((1, 3, 40, 50, -1, 0, 5), b"crop_border must be >= 0"),
                        ((1, 3, 40, 50, 20, 0, 5), b"nothing left after the crop"), ((1, 3, 16, 40, 3, 0, 5), b"at least 11 x 11"),
                        ((1, 3, 40, 50, 0, 0, 9), b"levels must be 1 .. 8"), ((1, 3, 40, 50, 0, 0, 0), b"levels must be 1 .. 8"),
                        ((4000, 3, 40, 50, 0, 0, 8), b"above 65535"), ((1, 3, 40, 50, 0, 2, 5), b"unknown flag")]:
        assert lib.dcpt_msssim_ws_bytes(*args) == 0
        assert lib.dcpt_msssim(1, 1, 1, 1, 1 << 30, *args, None) != 0 and words in lib.dcpt_last_error(), (args, lib.dcpt_last_error())
    for fn, ws, name in ((lib.dcpt_ssim_matlab, lib.dcpt_ssim_matlab_ws_bytes, b"ssim_matlab"), (None, lib.dcpt_imgrange_ws_bytes, b"imgrange")):
        for args, words in [((1, 2, 40, 50, 0, 0), b"C must be 1 or 3"), ((1, 3, 40, 50, -1, 0), b"crop_border must be >= 0"),
                            ((1, 3, 40, 50, 20, 0), b"nothing left after the crop"), ((30000, 3, 40, 50, 0, 0), b"above 65535"),
                            ((1, 3, 40, 50, 0, 2), b"unknown flag")]:
            assert ws(*args) == 0
            rc = fn(1, 1, 1, 1, 1 << 30, *args, None) if fn else lib.dcpt_imgrange(1, 1, 1, 1 << 30, *args, None)
            assert rc != 0 and words in lib.dcpt_last_error() and lib.dcpt_last_error().startswith(name), (args, lib.dcpt_last_error())
    assert lib.dcpt_msssim(None, None, None, None, 0, 1, 3, 40, 50, 0, 0, 5, None) != 0 and b"null" in lib.dcpt_last_error()
    need = lib.dcpt_ssim_matlab_ws_bytes(1, 3, 40, 50, 0, 0)
    assert lib.dcpt_ssim_matlab(1, 1, 1, 1, need - 1, 1, 3, 40, 50, 0, 0, None) != 0 and b"workspace too small" in lib.dcpt_last_error()
    assert lib.dcpt_msssim(1, 1, 1, None, 0, 1, 3, 40, 50, 0, 0, 5, None) != 0 and b"workspace too small" in lib.dcpt_last_error()
    assert lib.dcpt_imgrange(1, 1, 1, 8, 1, 3, 40, 50, 0, 0, None) != 0 and b"workspace too small" in lib.dcpt_last_error()
