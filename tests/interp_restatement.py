"""The arithmetic of dcpt_interp_fwd (include/dcpt_hip.h) restated in numpy float64, blind to the kernel: the taps of an axis for the three
modes, and the separable sum in the header's order -- columns inner, rows outer, both ascending, each step one multiply and one add.  (The
kernel fuses a step into one fma; the two differ by roundings of 2^-53 relative, far below the one fp32 rounding at the end.)"""
import math

import numpy as np

A = -0.75
MODES = ("area", "bilinear", "bicubic")


def c1(v):
    return ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0


def c2(v):
    return ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A


def axis_taps(mode, n, m, r):
    """per output index d of an axis with n source and m destination samples and ratio r: (list of source indices, list of weights)"""
    taps = []
    for d in range(m):
        if mode == "area":
            s, e = (d * n) // m, -((-(d + 1) * n) // m)
            taps.append((list(range(s, e)), [1.0 / (e - s)] * (e - s)))
        elif mode == "bilinear":
            src = max((d + 0.5) * r - 0.5, 0.0)
            i0 = min(int(math.floor(src)), n - 1)
            t = src - i0
            taps.append(([i0, min(i0 + 1, n - 1)], [1.0 - t, t]))
        elif mode == "bicubic":
            src = (d + 0.5) * r - 0.5
            i0 = int(math.floor(src))
            t = src - i0
            taps.append(([min(max(i0 - 1 + k, 0), n - 1) for k in range(4)], [c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)]))
        else:
            raise ValueError(mode)
    return taps


def geometry(in_size, size=None, scale_factor=None):
    """torch's rules: ((Ho, Wo), (ratio_h, ratio_w)); scale_factor gives floor(H sf) and 1 / sf, size gives H / Ho"""
    H, W = in_size
    if scale_factor is not None:
        sf = scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor, scale_factor)
        return (int(math.floor(H * sf[0])), int(math.floor(W * sf[1]))), (1.0 / sf[0], 1.0 / sf[1])
    out = size if isinstance(size, (tuple, list)) else (size, size)
    return tuple(out), (H / out[0], W / out[1])


def interp_f64(x, mode, size=None, scale_factor=None, clip=False, rounds=False):
    """x: (B, C, H, W) array; returns the float64 result before the cast to fp32"""
    x = np.asarray(x, dtype=np.float64)
    B, C, H, W = x.shape
    (Ho, Wo), (rh, rw) = geometry((H, W), size, scale_factor)
    cols, rows = axis_taps(mode, W, Wo, rw), axis_taps(mode, H, Ho, rh)
    inner = np.zeros((B, C, H, Wo))
    for j, (idx, w) in enumerate(cols):
        acc = np.zeros((B, C, H))
        for jb, wb in zip(idx, w):
            acc = acc + wb * x[:, :, :, jb]
        inner[:, :, :, j] = acc
    out = np.zeros((B, C, Ho, Wo))
    for i, (idx, w) in enumerate(rows):
        acc = np.zeros((B, C, Wo))
        for ia, wa in zip(idx, w):
            acc = acc + wa * inner[:, :, ia, :]
        out[:, :, i, :] = acc
    if clip:
        out = np.clip(out, 0.0, 1.0)
    if rounds:
        out = np.rint(255.0 * out) / 255.0
    return out


def interp_f32(x, mode, size=None, scale_factor=None, clip=False, rounds=False):
    return interp_f64(x, mode, size, scale_factor, clip, rounds).astype(np.float32)
