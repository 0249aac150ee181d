"""``filter2D``, ``usm_sharp`` and ``USMSharp`` of the reference's basicsr/utils/img_process_util.py on the fused blur kernel
(``dcpt_amd.functional.filter2d``, include/dcpt_hip.h dcpt_filter2d_fwd) and its host form (``basicsr.data.filter2d_host``).

The reference takes its Gaussian from ``cv2.getGaussianKernel`` and ``cv2.GaussianBlur``; cv2 is not a dependency of this package.  The
Gaussian here is the one cv2 documents for ``getGaussianKernel(ksize, sigma)``: ``sigma <= 0`` means ``0.3 * ((ksize - 1) * 0.5 - 1) +
0.8``, the taps are ``exp(-(i - (ksize - 1) / 2)^2 / (2 sigma^2))`` normalised to sum 1, in float64.  It has NOT been compared with cv2.
For ``ksize <= 7`` with ``sigma <= 0`` cv2 returns fixed tables instead of that formula; the case is refused here."""
import numpy as np
import torch

MAX_RADIUS = 51   # the largest kernel the blur kernel takes (dcpt_amd.functional.FILTER2D_MAX_K)


def gaussian_kernel1d(ksize, sigma=0):
    """the ``ksize`` float64 taps of the Gaussian documented for ``cv2.getGaussianKernel`` (not compared with cv2)"""
    if ksize % 2 == 0 or ksize < 1:
        raise ValueError(f"the Gaussian kernel size must be odd and positive, got {ksize}")
    if ksize > MAX_RADIUS:
        raise ValueError(f"a Gaussian kernel of {ksize} taps exceeds the blur kernel's limit of {MAX_RADIUS}")
    if sigma <= 0:
        if ksize <= 7:
            raise ValueError(f"cv2 uses fixed tables for a kernel size of {ksize} <= 7 with sigma <= 0; give a positive sigma")
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2
    taps = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return taps / taps.sum()


def _gaussian_kernel2d(radius, sigma=0):
    k = gaussian_kernel1d(radius, sigma)
    return np.outer(k, k).astype(np.float32)


def filter2D(img, kernel):
    """the reference's ``filter2D`` (a PyTorch ``cv2.filter2D``): ``img`` (b, c, h, w) fp32 device tensor, ``kernel`` (b, k, k) or
    (1, k, k); a correlation under reflect padding, one launch of the blur kernel (``dcpt_amd.functional.filter2d``)"""
    from dcpt_amd import functional as DF

    if kernel.size(-1) % 2 != 1:
        raise ValueError("Wrong kernel size")
    return DF.filter2d(img, kernel)


def usm_sharp(img, weight=0.5, radius=50, threshold=10):
    """USM sharpening of a numpy HWC float32 image in [0, 1] (reference :34-60): blur B of the image I by a ``radius`` Gaussian,
    sharp = clip(I + weight (I - B), 0, 1), mask = |I - B| * 255 > threshold blurred by the same Gaussian, out = mask sharp + (1 - mask) I.
    The blur is ``basicsr.data.filter2d_host`` with the Gaussian of this module (``cv2.GaussianBlur``'s default border is the same reflect
    rule; not compared with cv2)."""
    from basicsr.data import filter2d_host

    if radius % 2 == 0:
        radius += 1
    kernel = _gaussian_kernel2d(radius, 0)

    def blur(a):
        chw = np.ascontiguousarray(np.atleast_3d(a).transpose(2, 0, 1), dtype=np.float32)
        return filter2d_host(chw, kernel).transpose(1, 2, 0).reshape(a.shape)

    residual = img - blur(img)
    mask = (np.abs(residual) * 255 > threshold).astype("float32")
    soft_mask = blur(mask)
    sharp = np.clip(img + weight * residual, 0, 1)
    return soft_mask * sharp + (1 - soft_mask) * img


class USMSharp(torch.nn.Module):
    """the reference's ``USMSharp`` (:63-82): the buffer ``kernel`` (1, radius', radius') fp32, ``radius'`` = ``radius`` made odd, the
    outer product of the Gaussian of this module (the one ``cv2.getGaussianKernel(radius', sigma)`` documents; NOT compared with cv2, which
    is not installed).  ``radius' <= 7`` with ``sigma <= 0`` (cv2's fixed tables) and ``radius' > 51`` raise.  ``forward`` is two launches
    of the blur kernel and the reference's element-wise steps."""

    def __init__(self, radius=50, sigma=0):
        super().__init__()
        if radius % 2 == 0:
            radius += 1
        self.radius = radius
        self.register_buffer("kernel", torch.from_numpy(_gaussian_kernel2d(radius, sigma)).unsqueeze_(0))

    def forward(self, img, weight=0.5, threshold=10):
        residual = img - filter2D(img, self.kernel)
        soft = filter2D((residual.abs() * 255 > threshold).float(), self.kernel)   # the step mask, blurred
        sharp = (img + weight * residual).clip(0, 1)
        return soft * sharp + (1 - soft) * img
