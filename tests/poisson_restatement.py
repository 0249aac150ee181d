"""Kernel-blind restatement of dcpt_poisson_noise_fwd in numpy, written from the statement in include/dcpt_hip.h alone: the 8-bit levels and
their count, the Philox4x32-10 uniforms (the integer generator of tests/noise_restatement.py), the upward search in float64 and the output T
left in float64 (the kernel rounds it to fp32 once).  It never imports the package under test.

The search ``p = exp(-lam); s = p; k = 0; while s < u and k < 1023: k += 1; p = (p * lam) * R[k]; s = s + p`` does not depend on u except
through the comparison, and its sums S_0 <= S_1 <= ... never decrease (p >= 0).  So the k of a draw is the first index whose S_k is not
below u: ``cumulative`` runs the recurrence once per rate, numpy rounding every product and sum on its own as the header asks, and
``search`` looks u up in it.  ``search_literal`` is the loop as written, for the tests that compare the two."""
import numpy as np

from noise_restatement import philox4x32_10

KCAP = 1023
R = np.concatenate([[0.0], 1.0 / np.arange(1, KCAP + 1, dtype=np.float64)])   # R[k] = 1 / k, correctly rounded (R[0] unused)
NEAR_LEVEL = 1e-9      # (a): 255 v this close to a half-integer: the level, and with it U, could flip
NEAR_U = 2.0 ** -40    # (b): a partial sum this close to u: the k could flip (the module docstring of tests/test_gpu_poisson.py derives it)


def level(v):
    """(int) fmin(fmax(rint(255 v), 0), 255) of float64 values: half to even, NaN -> 0"""
    return np.fmin(np.fmax(np.rint(255.0 * np.asarray(v, dtype=np.float64)), 0.0), 255.0).astype(np.int64)


def uniforms(key, n):
    """the first n uniforms of the stream of the 64-bit ``key``: u_j of counter q belongs to value 4 q + j"""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    zero = np.zeros(nq, dtype=np.uint64)
    x = philox4x32_10([q, zero, zero, zero], (key & 0xFFFFFFFF, key >> 32))
    return np.stack([(v.astype(np.float64) + 0.5) * 2.0 ** -32 for v in x], axis=1).reshape(-1)[:n]


def cumulative(lam):
    """S[..., k] for k = 0..1023 of the rates ``lam`` (float64 array): the search's partial sums, each product and sum rounded on its own"""
    lam = np.asarray(lam, dtype=np.float64)
    S = np.empty(lam.shape + (KCAP + 1,), dtype=np.float64)
    p = np.exp(-lam)
    s = p.copy()
    S[..., 0] = s
    for k in range(1, KCAP + 1):
        p = (p * lam) * R[k]
        s = s + p
        S[..., k] = s
    return S


def search(S, u):
    """k of the draws ``u`` against ONE rate's sums S (1024 values): the first k with not (S_k < u), 1023 if there is none"""
    return np.minimum(np.searchsorted(S, u, side="left"), KCAP)


def search_literal(lam, u):
    """the loop of the header, one draw"""
    lam, u = np.float64(lam), np.float64(u)
    p = np.exp(-lam)
    s = p
    k = 0
    while s < u and k < KCAP:
        k += 1
        p = (p * lam) * R[k]
        s = s + p
    return k


def draws(key, lam, n):
    """the first n Poisson draws of rate ``lam`` on the stream of ``key``"""
    return search(cumulative(np.float64(lam)), uniforms(key, n))


class Result:
    """U, vals: int arrays [B];  k, lev (the count drawn and the level behind its rate): int64 [B, C, H, W];  T: float64 [B, C, H, W];  near_level, near_u: bool [B, C, H, W]"""


def poisson_noise(x, scale, key, gray=None, clip=False, rounds=False, noise_only=False):
    """x: (B, C, H, W) float32 array; scale, key, gray: B values"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    B, C, H, W = x.shape
    res = Result()
    res.U, res.vals = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    res.k, res.lev = np.zeros((B, C, H, W), dtype=np.int64), np.zeros((B, C, H, W), dtype=np.int64)
    res.T = np.empty((B, C, H, W), dtype=np.float64)
    res.near_level, res.near_u = np.zeros((B, C, H, W), dtype=bool), np.zeros((B, C, H, W), dtype=bool)
    for b in range(B):
        xb = x[b].astype(np.float64)
        if gray is not None and int(gray[b]) != 0:
            assert C in (1, 3)
            v = xb[0] if C == 1 else (0.2989 * xb[0] + 0.587 * xb[1]) + 0.114 * xb[2]   # (numpy rounds each product and sum)
            v = v.reshape(1, H, W)
        else:
            v = xb
        lev = level(v)
        present = np.unique(lev)
        U = len(present)
        vals = 1
        while vals < U:
            vals *= 2
        u = uniforms(key[b], lev.size).reshape(lev.shape)
        k = np.zeros(lev.shape, dtype=np.int64)
        near = np.zeros(lev.shape, dtype=bool)
        for l in present:
            S = cumulative(np.float64(int(l) * vals) / 255.0)
            at = lev == l
            kl = search(S, u[at])
            k[at] = kl
            near[at] = (np.abs(S[kl] - u[at]) <= NEAR_U) | ((kl > 0) & (np.abs(S[np.maximum(kl - 1, 0)] - u[at]) <= NEAR_U))
        t = np.float64(np.float32(scale[b])) * (k.astype(np.float64) / np.float64(vals) - lev.astype(np.float64) / 255.0)
        f = 255.0 * v
        half = np.abs(f - np.floor(f) - 0.5) <= NEAR_LEVEL
        res.U[b], res.vals[b] = U, vals
        res.k[b] = np.broadcast_to(k, (C, H, W))
        res.lev[b] = np.broadcast_to(lev, (C, H, W))
        res.near_u[b] = np.broadcast_to(near, (C, H, W))
        res.near_level[b] = np.broadcast_to(half, (C, H, W))
        res.T[b] = np.broadcast_to(t, (C, H, W)) if noise_only else xb + t
    if clip:
        res.T = np.clip(res.T, 0.0, 1.0)
    if rounds:
        res.T = np.rint(255.0 * res.T) / 255.0
    return res


def near_half(T, eps=1e-6):
    """the elements whose 255 T (before the rounding to the 8-bit grid) lies within eps of a half-integer: a last-bit difference of the
    fp64 library may move those to the neighbouring grid value"""
    v = 255.0 * T
    return np.abs(v - np.floor(v) - 0.5) <= eps
