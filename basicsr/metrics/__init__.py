"""METRIC_REGISTRY: cv2-free PSNR / SSIM with the reference's interface (basicsr/metrics/psnr_ssim.py:11-75 ``calculate_psnr``,
:113-183 ``calculate_ssim``, ``_ssim`` :483-512; ``reorder_image`` / ``to_y_channel`` of metric_util.py):

    calculate_psnr(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255)

``img`` / ``img2`` are float arrays in [0, 1] -- a batch (B,C,H,W) / (B,H,W,C), one image (C,H,W), or a 2-D map -- which are
scaled by ``image_range`` and ROUNDED to uint8 (uint16 for other ranges; ``image_range=1`` skips the quantisation), cropped,
optionally reduced to BT.601 luma, compared in float64 and averaged over the batch.  The reference's RGB->BGR flip
(cv2.cvtColor) only matters for the luma weights, which are applied here in the same B, G, R order.

Extension kept for callers that already hold quantised images: ``input_order`` "HWC" / "CHW" takes ONE image whose values are
already in [0, image_range] (no scaling, no rounding).

PSNR is pinned against the reference function itself (tests/golden/metrics.npz, oracle/make_golden.py::gen_metrics: the reference's
``calculate_psnr`` only needs ``cv2.cvtColor``'s channel flip, which a three-line module object provides).

SSIM stays RESTATEMENT-ONLY, deliberately: the arithmetic of the reference's ``_ssim`` (:483-512) lives in ``cv2.getGaussianKernel``
and ``cv2.filter2D``, and cv2 is not installed in the build image.  Running the reference function would therefore mean running it
on stand-ins for those two OpenCV routines written here -- the result would pin this file against its own author's reading of
OpenCV, not against the reference, so no such fixture is committed.  What is checked instead: ``calculate_ssim`` against an
independently written scipy implementation of the published formula (11 x 11 Gaussian, sigma 1.5, "valid" window, C1 = (0.01 L)^2,
C2 = (0.03 L)^2, float64; tests/test_plumbing_cpu.py::test_metrics_match_independent_implementations), and the acceptance gate of
``north_star`` is stated in PSNR (<= 0.01 dB), which IS pinned.

``calculate_psnr_device`` / ``calculate_ssim_device`` / ``MetricSums`` score BCHW tensors that are already on the device with the fused HIP
kernel of dcpt_amd/csrc/metrics.hip (same arithmetic, image_range 255 or 1); the host functions above stay the yardstick they are tested
against (tests/test_gpu_metrics.py).

``calculate_ssim_pt`` (reference psnr_ssim.py:436-480) is the differentiable SSIM of the losses: (B, C, H, W) fp32 device tensors in, the
per-image SSIM as a float64 tensor out, forward and gradient on the fused fp64 kernels of dcpt_amd/csrc/ssim_loss.hip.

``calculate_niqe`` / ``calculate_niqe_device`` / ``NiqeSums`` (reference basicsr/metrics/niqe.py) live in basicsr/metrics/niqe.py: the no-reference
metric, on the host in numpy float64 and on the fused fp64 kernels of dcpt_amd/csrc/niqe.hip, with one shared host finish.

``calculate_msssim`` (reference psnr_ssim.py:334-432), ``calculate_ssim_matlab`` (:201-330) and ``calculate_nrmse`` (:563-612) share the front
end above (``_images``) and are RESTATEMENT-ONLY for the reason given for SSIM: their arithmetic lives in ``cv2.filter2D`` /
``cv2.getGaussianKernel`` (MS-SSIM) or sits behind a module-level ``import cv2`` (the other two).  They are checked against independently
written scipy forms (tests/test_msmetrics_cpu.py).  ``calculate_msssim_device`` / ``calculate_ssim_matlab_device`` / ``calculate_nrmse_device``
and ``MetricSums(msssim=, ssim_matlab=, nrmse=)`` score device tensors with the kernels of dcpt_amd/csrc/metrics_ms.hip and finish with the
host functions' own finishing code.  ``calculate_psnr_pt`` (:79-110) is a torch expression on the tensors' own device."""
from copy import deepcopy

import numpy as np

from basicsr.utils.registry import METRIC_REGISTRY

from .niqe import NiqeSums, calculate_niqe, calculate_niqe_device

__all__ = ["calculate_metric", "calculate_psnr", "calculate_ssim", "calculate_psnr_device", "calculate_ssim_device", "MetricSums",
           "calculate_ssim_pt", "calculate_niqe", "calculate_niqe_device", "NiqeSums", "calculate_msssim", "calculate_ssim_matlab",
           "calculate_nrmse", "calculate_psnr_pt", "calculate_msssim_device", "calculate_ssim_matlab_device", "calculate_nrmse_device"]

METRIC_REGISTRY.register()(calculate_niqe)
METRIC_REGISTRY.register()(calculate_niqe_device)


def _reorder(img, input_order):
    """metric_util.reorder_image: anything -> (B, H, W, C)"""
    if input_order not in ("BHWC", "BCHW"):
        raise ValueError(f"Wrong input_order {input_order}. Supported input_orders are 'HWC' and 'CHW'")
    if img.ndim == 2:
        img = img[None, ..., None]
    if input_order == "BCHW":
        if img.ndim == 3:
            img = img.transpose(1, 2, 0)[None, ...]
        elif img.ndim == 4:
            img = img.transpose(0, 2, 3, 1)
    elif img.ndim == 3:
        img = img[None, ...]
    return img


def _to_y(img_rgb, image_range):
    """metric_util.to_y_channel on the BGR-flipped image (color_util.bgr2ycbcr, y_only): float32 in, float32 out, no rounding"""
    x = img_rgb[..., ::-1].astype(np.float32) / image_range
    if x.dtype != np.float32:
        x = x.astype(np.float32)
    y = (np.dot(x, [24.966, 128.553, 65.481]) + 16.0) / 255.0
    return y.astype(np.float32)[..., None] * image_range


def _images(img, img2, crop_border, input_order, test_y_channel, image_range):
    """yields the float64 (H, W, C) pairs the metric is evaluated on"""
    img, img2 = np.asarray(img), np.asarray(img2)
    assert img.shape == img2.shape, f"Image shapes are different: {img.shape}, {img2.shape}."
    legacy = input_order in ("HWC", "CHW")
    if legacy:
        if input_order == "CHW":
            img, img2 = img.transpose(1, 2, 0), img2.transpose(1, 2, 0)
        if img.ndim == 2:
            img, img2 = img[..., None], img2[..., None]
        batch = [(img, img2)]
    else:
        a, b = _reorder(img, input_order), _reorder(img2, input_order)
        batch = [(a[i], b[i]) for i in range(a.shape[0])]
    dtype = np.uint8 if image_range == 255 else np.uint16
    for x, y in batch:
        if not legacy and image_range != 1:
            x = (x * float(image_range)).round().astype(dtype)
            y = (y * float(image_range)).round().astype(dtype)
        if crop_border != 0:
            x = x[crop_border:-crop_border, crop_border:-crop_border, ...]
            y = y[crop_border:-crop_border, crop_border:-crop_border, ...]
        if test_y_channel and x.shape[-1] == y.shape[-1] == 3:
            x, y = _to_y(x, image_range), _to_y(y, image_range)
        yield x.astype(np.float64), y.astype(np.float64)


@METRIC_REGISTRY.register()
def calculate_psnr(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255, **kwargs):
    psnrs = []
    for x, y in _images(img, img2, crop_border, input_order, test_y_channel, image_range):
        mse = np.mean((x - y) ** 2)
        if mse == 0:
            return float("inf")
        psnrs.append(10.0 * np.log10(image_range * image_range / mse))
    return float(np.array(psnrs).mean())


def _gauss_kernel():
    """cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 sigma^2)), normalised to sum 1"""
    x = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(x ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def _filter_valid(img, k):
    """the 11x11 outer-product window as two 1-D 'valid' passes (cv2.filter2D then [5:-5, 5:-5] in the reference)"""
    h = np.apply_along_axis(lambda r: np.convolve(r, k, mode="valid"), 1, img)
    return np.apply_along_axis(lambda c: np.convolve(c, k, mode="valid"), 0, h)


def _ssim(img, img2, image_range=255):
    c1, c2 = (0.01 * image_range) ** 2, (0.03 * image_range) ** 2
    k = _gauss_kernel()
    mu1, mu2 = _filter_valid(img, k), _filter_valid(img2, k)
    mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = _filter_valid(img ** 2, k) - mu1_sq
    s2 = _filter_valid(img2 ** 2, k) - mu2_sq
    s12 = _filter_valid(img * img2, k) - mu12
    cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
    return (((2 * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map).mean()


@METRIC_REGISTRY.register()
def calculate_ssim(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255, **kwargs):
    ssims = []
    for x, y in _images(img, img2, crop_border, input_order, test_y_channel, image_range):
        for j in range(x.shape[2]):
            ssims.append(_ssim(x[..., j], y[..., j], image_range))
    return float(np.array(ssims).mean())


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # the reference's default (psnr_ssim.py:396)


def _ssim_cs(img, img2, image_range=255):
    """the reference's ``_ssim`` as ``calculate_msssim`` uses it: (ssim_map.mean(), cs_map.mean()); the arithmetic of ``_ssim`` above"""
    c1, c2 = (0.01 * image_range) ** 2, (0.03 * image_range) ** 2
    k = _gauss_kernel()
    mu1, mu2 = _filter_valid(img, k), _filter_valid(img2, k)
    mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = _filter_valid(img ** 2, k) - mu1_sq
    s2 = _filter_valid(img2 ** 2, k) - mu2_sq
    s12 = _filter_valid(img * img2, k) - mu12
    cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
    return (((2 * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map).mean(), cs_map.mean()


def _box_blur(a):
    """cv2.filter2D(a, -1, ones((2, 2)) / 4, anchor=(0, 0), borderType=BORDER_REFLECT) on (H, W, C): the mean of a[y][x], a[y][x+1],
    a[y+1][x], a[y+1][x+1], an index one past the last row / column reading the last one; the size is unchanged.  The order of the adds is
    fixed: 0.25 * ((a00 + a01) + (a10 + a11))."""
    a10 = np.concatenate([a[1:], a[-1:]], axis=0)
    a01 = np.concatenate([a[:, 1:], a[:, -1:]], axis=1)
    a11 = np.concatenate([a10[:, 1:], a10[:, -1:]], axis=1)
    return 0.25 * ((a + a01) + (a10 + a11))


def _msssim_of_means(ssims, css, weights):
    """the finish of ``calculate_msssim`` (reference :427-432) from the per-evaluation means (B, L) of the SSIM and CS maps: per image
    prod(cs[:L-1] ** w[:L-1]) * ssim[L-1] ** w[L-1] (NaN for a negative mean under a fractional weight, as numpy gives it), then the mean
    over the batch"""
    level = len(weights)
    results = []
    for s, c in zip(np.asarray(ssims, dtype=np.float64), np.asarray(css, dtype=np.float64)):
        results.append(np.prod(np.power(c[: level - 1], weights[: level - 1])) * (s[level - 1] ** weights[level - 1]))
    return float(np.array(results).mean())


@METRIC_REGISTRY.register()
def calculate_msssim(img, img2, crop_border, weights=None, image_range=255, input_order="BCHW", test_y_channel=False, **kwargs):
    """The reference's ``calculate_msssim`` (psnr_ssim.py:334-432), restatement-only (cv2; see the module docstring), quirks kept:

    * the scales are NOT decimated: between two evaluations both images pass through the 2 x 2 box filter ``_box_blur`` at full size;
    * the blur sits inside the reference's channel loop, so evaluation k = 0, 1, ... scores channel ``k mod C`` of the images after k blurs
      of every channel, and only evaluations 0 .. L - 1 (L = ``len(weights)``) enter the result: with the default five weights a 3-channel
      pair is scored on channels 0, 1, 2, 0, 1 at blur depths 0 .. 4;
    * per image the value is ``prod(cs[:L-1] ** weights[:L-1]) * ssim[L-1] ** weights[L-1]``, the metric its mean over the batch; a negative
      mean gives NaN.

    The window is the 11 x 11 "valid" Gaussian of ``calculate_ssim``; the cropped image must be at least 11 x 11."""
    weights = list(MSSSIM_WEIGHTS if weights is None else weights)
    level = len(weights)
    ssims, css = [], []
    for x, y in _images(img, img2, crop_border, input_order, test_y_channel, image_range):
        s_img, c_img = [], []
        for k in range(level):
            j = k % x.shape[2]
            s, c = _ssim_cs(x[..., j], y[..., j], image_range)
            s_img.append(s)
            c_img.append(c)
            if k < level - 1:
                x, y = _box_blur(x), _box_blur(y)
        ssims.append(s_img)
        css.append(c_img)
    return _msssim_of_means(ssims, css, weights)


def _ssim_matlab_map_mean(img, img2, image_range=255):
    """SSIM_MATLAB_Pytorch._ssim (reference :229-250) on one channel in float64: the window at every pixel under replicate padding of 5"""
    c1, c2 = (0.01 * image_range) ** 2, (0.03 * image_range) ** 2
    k = _gauss_kernel()
    x, y = np.pad(img, 5, mode="edge"), np.pad(img2, 5, mode="edge")
    mu1, mu2 = _filter_valid(x, k), _filter_valid(y, k)
    mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = _filter_valid(x ** 2, k) - mu1_sq
    s2 = _filter_valid(y ** 2, k) - mu2_sq
    s12 = _filter_valid(x * y, k) - mu12
    return (((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))).mean()


def _ssim_matlab_of_means(per_channel):
    """the finish of ``calculate_ssim_matlab`` from the per-(image, channel) map means (B, C'): the reference appends the last channel's
    value of every image a second time (:323-327) and averages all entries"""
    ssims = []
    for vals in np.asarray(per_channel, dtype=np.float64):
        ssims.extend(vals)
        ssims.append(vals[-1])
    return float(np.array(ssims).mean())


@METRIC_REGISTRY.register()
def calculate_ssim_matlab(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255, **kwargs):
    """The reference's ``calculate_ssim_matlab`` (psnr_ssim.py:201-330), restatement-only (the reference file imports cv2), quirks kept:

    * per channel the five moments go through the 11 x 11 Gaussian at EVERY pixel under replicate padding of 5, so the map has the cropped
      image's size and any size >= 1 x 1 is legal; the map ((2 mu12 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) is averaged;
    * per image the list is [ch0, ..., ch(C-1), ch(C-1)]: the last channel's value is appended twice; the metric is the mean of all entries.

    DELIBERATE DEVIATION: the reference runs its convolution in fp32 (``.float()``, ``Conv2d``); here everything is float64, like the MATLAB
    original the function cites.  The distance is measured in tests/test_msmetrics_cpu.py and recorded in DESIGN.md section 8."""
    per = []
    for x, y in _images(img, img2, crop_border, input_order, test_y_channel, image_range):
        per.append([_ssim_matlab_map_mean(x[..., j], y[..., j], image_range) for j in range(x.shape[2])])
    return _ssim_matlab_of_means(per)


def _nrmse_of_stats(mses, los, his):
    """the finish of ``calculate_nrmse`` (reference :607-612) from the per-image mean squared error and the minimum / maximum of the first
    image: sqrt(mse) / (max - min) averaged over the batch; the first image with rmse == 0 makes the whole call ``inf``; a constant first
    image divides by zero the way numpy does"""
    nrmses = []
    for mse, lo, hi in zip(mses, los, his):
        rmse = np.sqrt(np.float64(mse))
        if rmse == 0:
            return float("inf")
        nrmses.append(rmse / (np.float64(hi) - np.float64(lo)))
    return float(np.array(nrmses).mean())


@METRIC_REGISTRY.register()
def calculate_nrmse(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255, **kwargs):
    """The reference's ``calculate_nrmse`` (psnr_ssim.py:563-612), restatement-only (the reference file imports cv2): per image
    sqrt(mean((x - y)^2)) over all scored channels divided by ``x.max() - x.min()`` of the FIRST argument after the front end, averaged over
    the batch.  Quirks kept: the first image with rmse == 0 makes the whole call return ``inf``; a constant ``x`` divides by zero the way
    numpy does (``inf`` with a RuntimeWarning)."""
    mses, los, his = [], [], []
    for x, y in _images(img, img2, crop_border, input_order, test_y_channel, image_range):
        mses.append(np.mean((x - y) ** 2))
        los.append(x.min())
        his.append(x.max())
    return _nrmse_of_stats(mses, los, his)


@METRIC_REGISTRY.register()
def calculate_psnr_pt(img, img2, crop_border, test_y_channel=False, **kwargs):
    """The reference's ``calculate_psnr_pt`` (psnr_ssim.py:79-110): tensors (B, 3 / 1, H, W) in [0, 1], NO quantisation; cropped, optionally
    reduced to luma (``basicsr.utils.rgb2ycbcr_pt(y_only=True)``), compared in float64: 10 log10(1 / (mse + 1e-12)) per image.  Returns the
    float64 tensor (B,), not a float.  A torch expression on whatever device the tensors are on; nothing synchronises."""
    import torch

    from basicsr.utils import rgb2ycbcr_pt

    assert img.shape == img2.shape, f"Image shapes are different: {img.shape}, {img2.shape}."
    if crop_border != 0:
        img = img[:, :, crop_border:-crop_border, crop_border:-crop_border]
        img2 = img2[:, :, crop_border:-crop_border, crop_border:-crop_border]
    if test_y_channel and img.shape[1] == img2.shape[1] == 3:
        img, img2 = rgb2ycbcr_pt(img, y_only=True), rgb2ycbcr_pt(img2, y_only=True)
    mse = torch.mean((img.to(torch.float64) - img2.to(torch.float64)) ** 2, dim=[1, 2, 3])
    return 10.0 * torch.log10(1.0 / (mse + 1e-12))


class MetricSums:
    """Device-side PSNR / SSIM of a whole dataset (dcpt_amd.functional.image_metric_sums: one fused HIP kernel per call, no host sync):
    ``add(img, img2)`` takes (B, C, H, W) fp32 device tensors in [0, 1] and keeps the per-image sums on the device; ``result()`` copies
    them to the host in ONE transfer and returns ``{"psnr": [...], "ssim": [...]}`` with one value per ``add`` call -- what
    ``calculate_psnr`` / ``calculate_ssim`` return for that batch, finished with the same numpy expressions (``np.mean`` of the squared
    error, ``10 log10(L^2 / mse)``, ``inf`` on ``mse == 0``, the mean over images and over (image, channel)).

    ``msssim`` (with ``weights``, at most 8) / ``ssim_matlab`` / ``nrmse`` add the keys of those names (dcpt_amd.functional.msssim_sums,
    ssim_matlab_sums, image_range_minmax), one value per ``add`` call, each finished by the function the host metric finishes with
    (``_msssim_of_means``, ``_ssim_matlab_of_means``, ``_nrmse_of_stats``): NaN and ``inf`` behave as on the host.  With the defaults
    ``result()`` and ``pending()`` are what they were without them."""

    def __init__(self, crop_border=0, input_order="BCHW", test_y_channel=False, image_range=255, psnr=True, ssim=True, msssim=False,
                 weights=None, ssim_matlab=False, nrmse=False, **kwargs):
        if input_order != "BCHW":
            raise ValueError(f"the device metrics take BCHW tensors (input_order {input_order})")
        if image_range not in (255, 1):
            raise ValueError(f"image_range {image_range}: the device metrics know 255 and 1")
        self.crop_border, self.test_y_channel, self.image_range = int(crop_border), bool(test_y_channel), image_range
        self.psnr, self.ssim = bool(psnr), bool(ssim)
        self.msssim, self.ssim_matlab, self.nrmse = bool(msssim), bool(ssim_matlab), bool(nrmse)
        self.weights = list(MSSSIM_WEIGHTS if weights is None else weights)
        # per add(): (sse (B,) or None, ssim sums (B, C') or None, pixels per image, SSIM-map positions per channel,
        #             [(kind, device tensor)] of the further kinds in the order msssim, ssim_matlab, nrmse)
        self._parts = []

    def add(self, img, img2):
        from dcpt_amd import functional as DF

        args = (self.crop_border, self.test_y_channel, self.image_range)
        sse = sums = None
        if self.psnr or self.ssim or self.nrmse or not (self.msssim or self.ssim_matlab):   # (the squared error: PSNR and NRMSE share it)
            sse, sums = DF.image_metric_sums(img, img2, *args, ssim=self.ssim)
        more = []
        if self.msssim:
            more.append(("msssim", DF.msssim_sums(img, img2, *args, levels=len(self.weights))))
        if self.ssim_matlab:
            more.append(("ssim_matlab", DF.ssim_matlab_sums(img, img2, *args)))
        if self.nrmse:
            more.append(("nrmse", DF.image_range_minmax(img, *args)))
        b, c, h, w = img.shape
        hc, wc = h - 2 * self.crop_border, w - 2 * self.crop_border
        cp = 1 if (self.test_y_channel and c == 3) else c
        self._parts.append((sse, sums, hc * wc * cp, (hc - 10) * (wc - 10), more))

    def pending(self):
        """the device tensors ``result`` needs, flat, as 8-byte words (the exact int64 sums bit for bit): a caller that holds several
        accumulators concatenates them, transfers once and hands every accumulator its slice (``result(host)``)"""
        import torch

        return [t.reshape(-1).view(torch.int64) for sse, sums, _, _, more in self._parts for t in (sse, sums, *(m for _, m in more))
                if t is not None]

    def result(self, host=None):
        """``host``: the int64 numpy array of ``torch.cat(self.pending())`` if the caller made the transfer; else it is made here"""
        import torch

        out = {"psnr": [], "ssim": []}
        out.update({k: [] for k, on in (("msssim", self.msssim), ("ssim_matlab", self.ssim_matlab), ("nrmse", self.nrmse)) if on})
        if not self._parts:
            return out
        if host is None:
            host = torch.cat(self.pending()).cpu().numpy()   # one transfer
        pos = 0
        for sse, sums, npix, npos, more in self._parts:
            if sse is not None:
                raw = host[pos:pos + sse.numel()]
                pos += sse.numel()
                raw = raw if sse.dtype == torch.int64 else raw.view(np.float64)
                if self.psnr:
                    out["psnr"].append(_psnr_of_sums(raw, npix, self.image_range))
            if sums is not None:
                per_map = host[pos:pos + sums.numel()].view(np.float64) / npos
                pos += sums.numel()
                out["ssim"].append(float(per_map.mean()))
            for kind, t in more:   # each finished by the host metric's own finish
                vals = host[pos:pos + t.numel()].view(np.float64).reshape(tuple(t.shape))
                pos += t.numel()
                if kind == "msssim":
                    means = vals / npos
                    out[kind].append(_msssim_of_means(means[..., 0], means[..., 1], self.weights))
                elif kind == "ssim_matlab":
                    out[kind].append(_ssim_matlab_of_means(vals / (npix // vals.shape[1])))
                else:
                    out[kind].append(_nrmse_of_stats([np.float64(s) / npix for s in raw], vals[:, 0], vals[:, 1]))
        return out


def _psnr_of_sums(sse, npix, image_range):
    """calculate_psnr's loop over the images of one batch, from their squared-error sums"""
    psnrs = []
    for s in sse:
        mse = np.float64(s) / npix
        if mse == 0:
            return float("inf")
        psnrs.append(10.0 * np.log10(image_range * image_range / mse))
    return float(np.array(psnrs).mean())


@METRIC_REGISTRY.register()
def calculate_psnr_device(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255, **kwargs):
    """``calculate_psnr`` for (B, C, H, W) fp32 tensors on the device; returns a Python float (this call synchronises)"""
    acc = MetricSums(crop_border, input_order, test_y_channel, image_range, ssim=False)
    acc.add(img, img2)
    return acc.result()["psnr"][0]


@METRIC_REGISTRY.register()
def calculate_ssim_device(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255, **kwargs):
    """``calculate_ssim`` for (B, C, H, W) fp32 tensors on the device; returns a Python float (this call synchronises)"""
    acc = MetricSums(crop_border, input_order, test_y_channel, image_range, psnr=False)
    acc.add(img, img2)
    return acc.result()["ssim"][0]


@METRIC_REGISTRY.register()
def calculate_msssim_device(img, img2, crop_border, weights=None, image_range=255, input_order="BCHW", test_y_channel=False, **kwargs):
    """``calculate_msssim`` for (B, C, H, W) fp32 tensors on the device; returns a Python float (this call synchronises)"""
    acc = MetricSums(crop_border, input_order, test_y_channel, image_range, psnr=False, ssim=False, msssim=True, weights=weights)
    acc.add(img, img2)
    return acc.result()["msssim"][0]


@METRIC_REGISTRY.register()
def calculate_ssim_matlab_device(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255, **kwargs):
    """``calculate_ssim_matlab`` for (B, C, H, W) fp32 tensors on the device; returns a Python float (this call synchronises)"""
    acc = MetricSums(crop_border, input_order, test_y_channel, image_range, psnr=False, ssim=False, ssim_matlab=True)
    acc.add(img, img2)
    return acc.result()["ssim_matlab"][0]


@METRIC_REGISTRY.register()
def calculate_nrmse_device(img, img2, crop_border, input_order="BCHW", test_y_channel=False, image_range=255, **kwargs):
    """``calculate_nrmse`` for (B, C, H, W) fp32 tensors on the device; returns a Python float (this call synchronises)"""
    acc = MetricSums(crop_border, input_order, test_y_channel, image_range, psnr=False, ssim=False, nrmse=True)
    acc.add(img, img2)
    return acc.result()["nrmse"][0]


@METRIC_REGISTRY.register()
def calculate_ssim_pt(img, img2, crop_border, test_y_channel=False, image_range=255, **kwargs):
    """the reference's ``calculate_ssim_pt`` (psnr_ssim.py:436-480, ``_ssim_pth`` :515-559): images in [0, 1] of shape (B, 3 / 1, H, W),
    cropped, optionally reduced to luma, compared in float64 with C1 = (0.01 image_range)^2, C2 = (0.03 image_range)^2; returns the
    float64 tensor (B,) of per-image SSIM, differentiable with respect to ``img`` (dcpt_amd.functional.ssim_pt; nothing synchronises)"""
    from dcpt_amd import functional as DF

    return DF.ssim_pt(img, img2, crop_border, test_y_channel, image_range)


def calculate_metric(data, opt):
    opt = deepcopy(opt)
    return METRIC_REGISTRY.get(opt.pop("type"))(**data, **opt)
