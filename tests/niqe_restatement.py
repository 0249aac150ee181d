"""A kernel-blind numpy restatement of the reference's NIQE (basicsr/metrics/niqe.py) and ``imresize``
(basicsr/utils/matlab_functions.py), parameterised by the dtype it computes in: ``np.float64`` (what fp64 arithmetic itself loses) or
``np.longdouble`` (the truth T of tests/test_gpu_niqe.py).  It follows the reference line by line -- per-block loops, ``np.roll``, masks,
``argmin`` over the 9801-point grid -- and knows nothing of tiles, tables on a device or summation trees.

Two places state a formula differently from the reference's text, for the same value:
  * the moments are taken around the window's centre pixel, mu = p + sum w (x - p), var = sum w (x - p)^2 - (mu - p)^2.  The reference
    gets an exact 0 on a constant window from float32 rounding (its ``convolve`` returns float32, and 8-bit values survive that); in float64
    or longdouble only this form gives the exact 0 that its NaN pattern on flat blocks hinges on.
  * the symmetric padded copies of ``imresize`` are an index map (-1 -> 0, n -> n - 1).
The crop is spatial (H and W of every plane), the departure from the reference that basicsr/metrics/niqe.py documents.  The Gamma function is
``math.gamma`` in float64 for every dtype: it enters only the features, never the sums, MSCN planes or resize outputs the kernels are held to."""
import math

import numpy as np

SHIFTS = ([0, 1], [1, 0], [1, 1], [1, -1])


def window(dtype):
    i = np.arange(-3, 4).astype(dtype)
    g = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2 * (dtype(7) / dtype(6)) ** 2))
    return g / g.sum()


# ---- imresize --------------------------------------------------------------------------------------
def _cubic(x):
    absx = np.abs(x)
    absx2, absx3 = absx ** 2, absx ** 3
    return (1.5 * absx3 - 2.5 * absx2 + 1) * (absx <= 1) + (-0.5 * absx3 + 2.5 * absx2 - 4 * absx + 2) * ((absx > 1) & (absx <= 2))


def weights_indices(in_length, out_length, scale, antialiasing, dtype):
    """matlab_functions.py:17-70 without the column trimming: (1-based index matrix, weights), both [out][p]"""
    kernel_width = dtype(4)
    scale = dtype(scale)
    if scale < 1 and antialiasing:
        kernel_width = kernel_width / scale
    x = np.arange(1, out_length + 1).astype(dtype)
    u = x / scale + dtype(0.5) * (1 - 1 / scale)
    left = np.floor(u - kernel_width / 2)
    p = math.ceil(kernel_width) + 2
    indices = left[:, None] + np.arange(p).astype(dtype)[None, :]
    dist = u[:, None] - indices
    weights = scale * _cubic(dist * scale) if (scale < 1 and antialiasing) else _cubic(dist)
    return indices.astype(np.int64), weights / weights.sum(axis=1, keepdims=True)


def _symmetric(idx1, n):
    i = idx1 - 1
    i = np.where(i < 0, -i - 1, i)
    i = np.where(i >= n, 2 * n - 1 - i, i)
    return np.clip(i, 0, n - 1)   # (only taps of weight zero ever need the clip)


def imresize_planes(planes, scale, antialiasing=True, dtype=np.float64):
    """[P][H][W] -> [P][ceil(H scale)][ceil(W scale)] in ``dtype``: the H pass, then the W pass (matlab_functions.py:148-177)"""
    planes = np.asarray(planes).astype(dtype)
    _, h, w = planes.shape
    oh, ow = math.ceil(h * scale), math.ceil(w * scale)
    ih, wh = weights_indices(h, oh, scale, antialiasing, dtype)
    iw, ww = weights_indices(w, ow, scale, antialiasing, dtype)
    out1 = np.zeros((planes.shape[0], oh, w), dtype=dtype)
    for i in range(oh):
        rows = planes[:, _symmetric(ih[i], h), :]                 # [P][p][W]
        out1[:, i, :] = (rows * wh[i][None, :, None]).sum(axis=1)
    out2 = np.zeros((planes.shape[0], oh, ow), dtype=dtype)
    for j in range(ow):
        cols = out1[:, :, _symmetric(iw[j], w)]                   # [P][oh][p]
        out2[:, :, j] = (cols * ww[j][None, None, :]).sum(axis=2)
    return out2


# ---- NIQE ------------------------------------------------------------------------------------------
def mscn(img, dtype):
    """niqe.py:121-129 on one plane [H][W], borders replicated (mode="nearest"), moments around the centre pixel"""
    img = img.astype(dtype)
    g = window(dtype)
    h, w = img.shape
    pad = np.pad(img, 3, mode="edge")
    s, q = np.zeros_like(img), np.zeros_like(img)
    for a in range(7):
        for b in range(7):
            d = pad[a:a + h, b:b + w] - img
            s = s + g[a, b] * d
            q = q + g[a, b] * d * d
    mu = img + s
    sigma = np.sqrt(np.abs(q - np.square(mu - img)))
    return -s / (sigma + 1)   # (img - mu, without rounding p + s first)


def six(x):
    """the sums estimate_aggd_param needs of one map (niqe.py:31-34)"""
    x = x.flatten()
    return [float((x < 0).sum()), (x[x < 0] ** 2).sum(), float((x > 0).sum()), (x[x > 0] ** 2).sum(), np.abs(x).sum(), (x ** 2).sum()]


def block_maps(n, bs):
    """yields (block index in the reference's order, [the block, its four rolled products]) of one MSCN plane"""
    nbh, nbw = n.shape[0] // bs, n.shape[1] // bs
    k = 0
    for idx_w in range(nbw):
        for idx_h in range(nbh):
            block = n[idx_h * bs:(idx_h + 1) * bs, idx_w * bs:(idx_w + 1) * bs]
            yield k, [block] + [block * np.roll(block, s, axis=(0, 1)) for s in SHIFTS]
            k += 1


def pipeline(img, crop_border=0, dtype=np.float64):
    """(B, C, H, W) float image in [0, 1] -> {"mscn1" [P][Hc][Wc], "img2" [P][Hc/2][Wc/2] (in [0, 1]), "mscn2", "stats" [P][nblk][2][5][6]},
    everything in ``dtype``"""
    img = np.asarray(img)
    x = (img.astype(np.float32) * 255.0).round().reshape(-1, *img.shape[2:])
    c = int(crop_border)
    if c:
        x = x[:, c:-c, c:-c]
    nbh, nbw = x.shape[1] // 96, x.shape[2] // 96
    x = x[:, :nbh * 96, :nbw * 96].astype(dtype)
    n1 = np.stack([mscn(p, dtype) for p in x])
    img2 = imresize_planes(x / dtype(255), 0.5, True, dtype)
    n2 = np.stack([mscn(p * dtype(255), dtype) for p in img2])
    stats = np.zeros((x.shape[0], nbh * nbw, 2, 5, 6), dtype=dtype)
    for p in range(x.shape[0]):
        for s, (n, bs) in enumerate(((n1[p], 96), (n2[p], 48))):
            for k, maps in block_maps(n, bs):
                for m, v in enumerate(maps):
                    stats[p, k, s, m] = six(v)
    return {"mscn1": n1, "img2": img2, "mscn2": n2, "stats": stats}


_GAM = np.arange(0.2, 10.001, 0.001)
_R_GAM = None


def _r_gam():
    global _R_GAM
    if _R_GAM is None:
        rec = np.reciprocal(_GAM)
        _R_GAM = np.array([math.gamma(2 * v) ** 2 / (math.gamma(v) * math.gamma(3 * v)) for v in rec])
    return _R_GAM


def estimate_aggd_param(block):
    """niqe.py:14-43, float64"""
    block = np.asarray(block, dtype=np.float64).flatten()
    with np.errstate(invalid="ignore", divide="ignore"):
        neg, pos = block[block < 0], block[block > 0]
        left_std = np.sqrt(np.float64(np.sum(neg ** 2)) / len(neg))
        right_std = np.sqrt(np.float64(np.sum(pos ** 2)) / len(pos))
        gammahat = left_std / right_std
        rhat = (np.mean(np.abs(block))) ** 2 / np.mean(block ** 2)
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
        alpha = _GAM[np.argmin((_r_gam() - rhatnorm) ** 2)]
        f = np.sqrt(math.gamma(1 / alpha) / math.gamma(3 / alpha))
    return alpha, left_std * f, right_std * f


def compute_feature(maps):
    alpha, bl, br = estimate_aggd_param(maps[0])
    feat = [alpha, (bl + br) / 2]
    for m in maps[1:]:
        alpha, bl, br = estimate_aggd_param(m)
        feat.extend([alpha, (br - bl) * (math.gamma(2 / alpha) / math.gamma(1 / alpha)), bl, br])
    return feat


def features(parts):
    """``pipeline`` output -> the reference's distparam rows [P][nblk][36] (float64)"""
    n1, n2 = parts["mscn1"], parts["mscn2"]
    rows = []
    for p in range(n1.shape[0]):
        f1 = [compute_feature(maps) for _, maps in block_maps(n1[p], 96)]
        f2 = [compute_feature(maps) for _, maps in block_maps(n2[p], 48)]
        rows.append(np.concatenate([np.array(f1), np.array(f2)], axis=1))
    return np.array(rows)


def score(distparam, mu_pris_param, cov_pris_param):
    """niqe.py:147-164 for one plane's rows"""
    with np.errstate(invalid="ignore"):
        mu_distparam = np.nanmean(distparam, axis=0)
    cov_distparam = np.cov(distparam[~np.isnan(distparam).any(axis=1)], rowvar=False)
    invcov = np.linalg.pinv((cov_pris_param + cov_distparam) / 2)
    d = mu_pris_param - mu_distparam
    return float(np.squeeze(np.sqrt(d @ invcov @ d.T)))


def niqe(img, crop_border, mu_pris_param, cov_pris_param, dtype=np.float64):
    rows = features(pipeline(img, crop_border, dtype))
    return float(np.mean([score(r, mu_pris_param, cov_pris_param) for r in rows]))


# ---- fixture codecs (tests/golden/niqe.npz, tools/make_golden_niqe.py) ---------------------------------
# Both are lossless re-arrangements that let the npz's deflate see the redundancy: an 8-bit image as differences along W modulo 256, a
# float32 array as its four byte planes.
def encode_planes(planes):
    return np.diff(planes, axis=-1, prepend=np.zeros(planes.shape[:-1] + (1,), dtype=np.uint8)).astype(np.uint8)


def decode_planes(dx):
    return np.cumsum(dx, axis=-1, dtype=np.uint8)


def encode_f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.ascontiguousarray(np.moveaxis(a.view(np.uint8).reshape(a.shape + (4,)), -1, 0))


def decode_f32(b):
    return np.ascontiguousarray(np.moveaxis(b, 0, -1)).view(np.float32)[..., 0]
