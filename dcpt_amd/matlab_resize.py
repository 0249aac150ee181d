"""The tap tables of MATLAB's bicubic ``imresize`` as the reference builds them (basicsr/utils/matlab_functions.py:17-86,
``calculate_weights_indices``), in float64 numpy, and their evaluation on the host.  The tables feed dcpt_imresize_fwd
(dcpt_amd.functional.imresize); the host evaluation serves numpy arrays and CPU tensors (basicsr.utils.matlab_functions.imresize).

Differences from the reference's function, none of which moves a result: indices are 0-based first taps instead of a full index matrix
shifted by the padding; the all-zero first / last columns are kept (a zero-weight tap is harmless); the symmetric padding is an index map
(-1 -> 0, -2 -> 1, n -> n - 1, ...).  Where a reflected index of a tap that carries weight would leave the input -- the input is shorter
than the kernel reaches -- ``ValueError`` is raised; the reference fails there with a shape error."""
import math

import numpy as np

__all__ = ["cubic", "weights_indices", "out_length", "reflect_index", "resize_planes"]


def cubic(x):
    absx = np.abs(x)
    absx2, absx3 = absx ** 2, absx ** 3
    return (1.5 * absx3 - 2.5 * absx2 + 1) * (absx <= 1) + (-0.5 * absx3 + 2.5 * absx2 - 4 * absx + 2) * ((absx > 1) & (absx <= 2))


def out_length(in_length, scale):
    return math.ceil(in_length * scale)


def weights_indices(in_length, scale, antialiasing=True, kernel_width=4):
    """-> (first, weights): ``first`` int32 [out] the 0-based first tap of every output sample (may be negative), ``weights`` float64
    [out][K] with rows summing to 1; tap k of output i reads input ``reflect_index(first[i] + k)``"""
    in_length = int(in_length)
    n_out = out_length(in_length, scale)
    if in_length < 1 or n_out < 1:
        raise ValueError(f"imresize: nothing to resize (length {in_length}, scale {scale})")
    shrink = scale < 1 and antialiasing
    if shrink:
        kernel_width = kernel_width / scale
    x = np.arange(1, n_out + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - kernel_width / 2)
    p = math.ceil(kernel_width) + 2
    indices = left[:, None] + np.arange(p, dtype=np.float64)[None, :]   # 1-based
    dist = u[:, None] - indices
    weights = scale * cubic(dist * scale) if shrink else cubic(dist)
    weights = weights / weights.sum(axis=1, keepdims=True)
    first = (left - 1).astype(np.int64)
    used = weights != 0
    idx0 = first[:, None] + np.arange(p)[None, :]
    lo, hi = int(idx0[used].min()), int(idx0[used].max())
    if -lo > in_length or hi > 2 * in_length - 1:
        raise ValueError(f"imresize: an input of length {in_length} is shorter than the kernel reaches at scale {scale} "
                         f"(taps {lo}..{hi}; the symmetric extension covers {-in_length}..{2 * in_length - 1})")
    return first.astype(np.int32), np.ascontiguousarray(weights)


def reflect_index(idx, n):
    """the reference's symmetric padded copy as an index map; clamped like the kernel for taps of weight zero beyond one reflection"""
    idx = np.where(idx < 0, -idx - 1, idx)
    idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    return np.clip(idx, 0, n - 1)


def resize_planes(planes, scale, antialiasing=True):
    """float64 evaluation of the tables on planes [P][H][W]: the H pass, then the W pass, taps added in table order"""
    planes = np.asarray(planes, dtype=np.float64)
    _, h, w = planes.shape
    fh, wh = weights_indices(h, scale, antialiasing)
    fw, ww = weights_indices(w, scale, antialiasing)
    t = np.zeros((planes.shape[0], len(fh), w))
    for k in range(wh.shape[1]):
        t += wh[None, :, k, None] * planes[:, reflect_index(fh + k, h), :]
    y = np.zeros((planes.shape[0], len(fh), len(fw)))
    for k in range(ww.shape[1]):
        y += ww[None, None, :, k] * t[:, :, reflect_index(fw + k, w)]
    return y
