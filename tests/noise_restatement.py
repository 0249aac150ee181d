"""Kernel-blind restatement of dcpt_gauss_noise_fwd in numpy, written from the statement in include/dcpt_hip.h alone: Philox4x32-10 in
uint32 / uint64 integers, the Box-Muller transform in float64, and the output T left in float64 (the kernel rounds it to fp32 once).  It
never imports the package under test."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars; returns the four uint32 output arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & MASK, p1 >> S32, p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def normals(key, n):
    """the first n values of the stream of the 64-bit ``key`` as float64"""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    zero = np.zeros(nq, dtype=np.uint64)
    x = philox4x32_10([q, zero, zero, zero], (key & 0xFFFFFFFF, key >> 32))
    u = [(v.astype(np.float64) + 0.5) * 2.0 ** -32 for v in x]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    out = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1).reshape(-1)
    return out[:n]


def gauss_noise(x, sigma, key, gray=None, clip=False, rounds=False, noise_only=False):
    """x: (B, C, H, W) float32 array (values only matter without noise_only); sigma, key, gray: B values.  Returns T as float64."""
    x = np.asarray(x)
    B, C, H, W = x.shape
    out = np.empty((B, C, H, W), dtype=np.float64)
    for b in range(B):
        if gray is not None and int(gray[b]) != 0:
            n = np.broadcast_to(normals(key[b], H * W).reshape(1, H, W), (C, H, W))
        else:
            n = normals(key[b], C * H * W).reshape(C, H, W)
        t = np.float64(np.float32(sigma[b])) / 255.0 * n
        out[b] = t if noise_only else x[b].astype(np.float64) + t
    if clip:
        out = np.clip(out, 0.0, 1.0)
    if rounds:
        out = np.rint(255.0 * out) / 255.0
    return out


def near_half(x, sigma, key, gray=None, clip=False, noise_only=False, eps=1e-6):
    """the elements whose 255 T (before the rounding to the 8-bit grid) lies within eps of a half-integer: a last-bit difference of the
    fp64 library may move those to the neighbouring grid value"""
    v = 255.0 * gauss_noise(x, sigma, key, gray, clip=clip, rounds=False, noise_only=noise_only)
    return np.abs(v - np.floor(v) - 0.5) <= eps
