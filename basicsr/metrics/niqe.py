"""NIQE with the reference's interface (basicsr/metrics/niqe.py): ``calculate_niqe`` on the host in numpy float64 -- the yardstick --,
``calculate_niqe_device`` / ``NiqeSums`` on the fused fp64 kernels of dcpt_amd/csrc/niqe.hip, and the finish both share.

What the reference computes, and this does too: ``(img * 255).round()`` of a float image in [0, 1]; every (b, c) plane scored on its own and
the scores averaged; per plane the crop to whole 96 x 96 blocks, then at two scales the 7 x 7 Gaussian moments (borders replicated), the
MSCN image ``(img - mu) / (sigma + 1)`` and per block (column-major order) 18 AGGD features of the block and of its products with
``np.roll(block, s, axis=(0, 1))``, s in [0,1], [1,0], [1,1], [1,-1]; the scale-2 image is ``imresize(img / 255, 0.5) * 255``; the finish is
``nanmean`` over blocks, ``np.cov`` of the NaN-free rows, ``pinv((cov_pris + cov) / 2)``, the quadratic form and ``sqrt``.

The pixel work ends in six sums per map -- count and sum of squares of the negative elements, the same of the positive ones, sum |x| and
sum x^2 -- an array [P][nblk][2][5][6]; ``features_from_stats`` / ``niqe_from_stats`` turn it into the feature rows and the score with the
reference's NaN semantics: a block that is exactly zero has empty sides, its row carries 13 NaN of 18 per scale and alpha = 0.2 (``argmin`` of
an all-NaN array is 0), and those entries still enter the column-wise ``nanmean``.

The moments are formed around the window's centre pixel p (mu = p + sum w (x - p), var = sum w (x - p)^2 - (mu - p)^2), so a constant window
gives exactly 0, as the reference's float32 arithmetic does on 8-bit images; the raw sum w x^2 - mu^2 in float64 would not.  The 7 x 7 window
is computed (exp(-(i^2 + j^2) / (2 (7/6)^2)), normalised: the reference's stored window to 1.4e-17).  The Gamma function is ``math.gamma``.

Departures from the reference, both deliberate: ``crop_border`` crops H and W of every plane (the reference slices the first two axes of the
squeezed array, so a B * C > 1 input with a crop gives NaN), and a single plane (B = C = 1) is scored (the reference iterates over its rows
and asserts).  The Y / gray conversion is commented out in the reference and absent here: ``convert_to`` is accepted and ignored.

The pristine model (``mu_pris_param`` (1, 36), ``cov_pris_param`` (36, 36)) is data the user supplies: ``pris_params=`` (a path to an npz, or
a mapping with the two arrays), else the environment variable ``DCPT_NIQE_PRIS_PARAMS``, else ``niqe_pris_params.npz`` next to this file."""
import math
import os

import numpy as np

__all__ = ["calculate_niqe", "calculate_niqe_device", "NiqeSums", "niqe_block_stats", "features_from_stats", "niqe_from_stats",
           "load_pris_params", "gaussian_window"]

BLOCK = 96
_SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def gaussian_window():
    i = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def load_pris_params(pris_params=None):
    """-> (mu_pris_param (1, 36), cov_pris_param (36, 36)) float64"""
    if pris_params is not None and not isinstance(pris_params, (str, os.PathLike)):
        return (np.asarray(pris_params["mu_pris_param"], dtype=np.float64).reshape(1, -1),
                np.asarray(pris_params["cov_pris_param"], dtype=np.float64))
    beside = os.path.join(os.path.dirname(os.path.abspath(__file__)), "niqe_pris_params.npz")
    path = pris_params or os.environ.get("DCPT_NIQE_PRIS_PARAMS") or (beside if os.path.isfile(beside) else None)
    if path is None:
        raise FileNotFoundError("calculate_niqe: the pristine NIQE parameters were not found.  Pass pris_params= (the metric's yml key "
                                "`pris_params`), set DCPT_NIQE_PRIS_PARAMS, or put niqe_pris_params.npz (mu_pris_param, cov_pris_param) "
                                f"at {beside}")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"calculate_niqe: the pristine NIQE parameters {path!r} do not exist")
    with np.load(path) as f:
        return np.asarray(f["mu_pris_param"], dtype=np.float64).reshape(1, -1), np.asarray(f["cov_pris_param"], dtype=np.float64)


# ---- geometry / input checks ---------------------------------------------------------------------
def _geometry(shape, crop_border, input_order):
    if input_order != "BCHW":
        raise ValueError(f"calculate_niqe takes BCHW images only (input_order {input_order!r})")
    if len(shape) != 4:
        raise ValueError(f"calculate_niqe: expected a (B, C, H, W) image, got {tuple(shape)}")
    crop = int(crop_border)
    if crop < 0:
        raise ValueError(f"calculate_niqe: crop_border must be >= 0 (got {crop_border})")
    b, c, h, w = (int(v) for v in shape)
    nbh, nbw = max(h - 2 * crop, 0) // BLOCK, max(w - 2 * crop, 0) // BLOCK
    if b * c < 1 or nbh * nbw < 2:
        raise ValueError(f"calculate_niqe: a plane needs at least two whole {BLOCK} x {BLOCK} blocks (the covariance over blocks is "
                         f"undefined otherwise); {h} x {w} with crop_border {crop} holds {nbh * nbw}")
    return b * c, crop, nbh, nbw


# ---- the pixel work on the host --------------------------------------------------------------------
def _mscn(img):
    """img [P][H][W] float64 -> the MSCN planes, moments around the centre pixel, borders replicated"""
    g = gaussian_window()
    h, w = img.shape[1:]
    pad = np.pad(img, ((0, 0), (3, 3), (3, 3)), mode="edge")
    s, q = np.zeros_like(img), np.zeros_like(img)
    for a in range(7):
        for b in range(7):
            d = pad[:, a:a + h, b:b + w] - img
            wd = g[a, b] * d
            s += wd
            q += wd * d
    return -s / (np.sqrt(np.abs(q - s * s)) + 1.0)


def _six(x):
    """x [..., bs, bs] -> [..., 6]"""
    x2 = x * x
    neg, pos = x < 0, x > 0
    ax = (-2, -1)
    return np.stack([neg.sum(ax).astype(np.float64), (x2 * neg).sum(ax), pos.sum(ax).astype(np.float64), (x2 * pos).sum(ax),
                     np.abs(x).sum(ax), x2.sum(ax)], axis=-1)


def _block_stats(n, bs):
    """MSCN planes [P][H][W] -> [P][nblk][5][6], blocks column-major"""
    p, h, w = n.shape
    nbh, nbw = h // bs, w // bs
    blocks = n.reshape(p, nbh, bs, nbw, bs).transpose(0, 3, 1, 2, 4).reshape(p, nbw * nbh, bs, bs)
    maps = [blocks] + [blocks * np.roll(blocks, s, axis=(2, 3)) for s in _SHIFTS]
    return np.stack([_six(m) for m in maps], axis=2)


def niqe_block_stats(img, crop_border=0, input_order="BCHW", parts=False):
    """the host form of dcpt_amd.functional.niqe_stats: (B, C, H, W) float array in [0, 1] -> [P][nblk][2][5][6] float64; with ``parts``
    also the intermediates {"mscn1", "img2", "mscn2"} (img2: the resize output in [0, 1])"""
    from dcpt_amd.matlab_resize import resize_planes

    img = np.asarray(img)
    p, crop, nbh, nbw = _geometry(img.shape, crop_border, input_order)
    x = (img.astype(np.float32) * 255.0).round().astype(np.float64).reshape(p, *img.shape[2:])
    x = x[:, crop:crop + nbh * BLOCK, crop:crop + nbw * BLOCK]
    n1 = _mscn(x)
    x2 = resize_planes(x / 255.0, 0.5, True)
    n2 = _mscn(x2 * 255.0)
    stats = np.stack([_block_stats(n1, BLOCK), _block_stats(n2, BLOCK // 2)], axis=2)
    return (stats, {"mscn1": n1, "img2": x2, "mscn2": n2}) if parts else stats


# ---- the finish (shared by the host and the device form) -----------------------------------------------
_GRID = None


def _gamma_grid():
    """gam = arange(0.2, 10.001, 0.001), r_gam = G(2/g)^2 / (G(1/g) G(3/g)) and the three Gamma columns"""
    global _GRID
    if _GRID is None:
        gam = np.arange(0.2, 10.001, 0.001)
        rec = np.reciprocal(gam)
        g1 = np.array([math.gamma(v) for v in rec])
        g2 = np.array([math.gamma(v) for v in rec * 2])
        g3 = np.array([math.gamma(v) for v in rec * 3])
        a1 = np.array([math.gamma(1 / a) for a in gam])   # the arguments of estimate_aggd_param's last lines: 1 / alpha, not reciprocal * k
        a2 = np.array([math.gamma(2 / a) for a in gam])
        a3 = np.array([math.gamma(3 / a) for a in gam])
        r_gam = np.square(g2) / (g1 * g3)
        _GRID = (gam, r_gam, a1, a2, a3, bool(np.all(np.diff(r_gam) > 0)))
    return _GRID


def _argmin_grid(rhatnorm):
    """np.argmin((r_gam - rhatnorm) ** 2) for every entry of ``rhatnorm``; 0 where it is NaN, as np.argmin of an all-NaN array"""
    gam, r_gam, _, _, _, increasing = _gamma_grid()
    flat = rhatnorm.reshape(-1)
    pos = np.zeros(flat.shape, dtype=np.int64)
    ok = ~np.isnan(flat)
    v = flat[ok]
    if increasing:   # the minimum of the squared distance lies next to the insertion point: compare the candidates with the same expression
        at = np.searchsorted(r_gam, v)
        cand = np.clip(at[:, None] + np.arange(-2, 3)[None, :], 0, len(r_gam) - 1)
        cand.sort(axis=1)
        d = (r_gam[cand] - v[:, None]) ** 2
        pos[ok] = cand[np.arange(len(v)), np.argmin(d, axis=1)]   # (first minimum, lowest index first: np.argmin's tie rule)
    else:
        pos[ok] = [int(np.argmin((r_gam - t) ** 2)) for t in v]
    return pos.reshape(rhatnorm.shape)


def features_from_stats(stats):
    """[P][nblk][2][5][6] sums -> the reference's ``distparam`` rows [P][nblk][36]"""
    stats = np.asarray(stats, dtype=np.float64)
    p, nblk = stats.shape[:2]
    gam, _, a1, a2, a3, _ = _gamma_grid()
    n = np.array([BLOCK * BLOCK, (BLOCK // 2) ** 2], dtype=np.float64)[None, None, :, None]
    cn, sn, cp, sp, sabs, ssq = (stats[..., k] for k in range(6))
    with np.errstate(invalid="ignore", divide="ignore"):
        left_std, right_std = np.sqrt(sn / cn), np.sqrt(sp / cp)   # (np.mean of an empty selection: NaN)
        gammahat = left_std / right_std
        rhat = (sabs / n) ** 2 / (ssq / n)
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
        pos = _argmin_grid(rhatnorm)
        alpha = gam[pos]
        scale = np.sqrt(a1[pos] / a3[pos])
        beta_l, beta_r = left_std * scale, right_std * scale
        mean = (beta_r - beta_l) * (a2[pos] / a1[pos])
    feat = np.empty((p, nblk, 2, 18))
    feat[..., 0] = alpha[..., 0]
    feat[..., 1] = (beta_l[..., 0] + beta_r[..., 0]) / 2
    for m in range(1, 5):
        o = 2 + 4 * (m - 1)
        feat[..., o], feat[..., o + 1], feat[..., o + 2], feat[..., o + 3] = alpha[..., m], mean[..., m], beta_l[..., m], beta_r[..., m]
    return feat.reshape(p, nblk, 36)


def niqe_from_stats(stats, mu_pris_param, cov_pris_param):
    """the per-plane NIQE values [P] of the sums [P][nblk][2][5][6] (niqe.py:147-164)"""
    out = []
    for distparam in features_from_stats(stats):
        with np.errstate(invalid="ignore"):
            mu_distparam = np.nanmean(distparam, axis=0)
        distparam_no_nan = distparam[~np.isnan(distparam).any(axis=1)]
        cov_distparam = np.cov(distparam_no_nan, rowvar=False)
        invcov_param = np.linalg.pinv((cov_pris_param + cov_distparam) / 2)
        d = mu_pris_param - mu_distparam
        out.append(float(np.squeeze(np.sqrt(np.matmul(np.matmul(d, invcov_param), np.transpose(d))))))
    return np.array(out)


# ---- the public forms --------------------------------------------------------------------------------------
def calculate_niqe(img, crop_border, input_order="BCHW", convert_to="y", pris_params=None, **kwargs):
    """NIQE of a float (B, C, H, W) array in [0, 1] on the host: the mean over the B * C planes.  ``img2`` (the validation loop passes the
    ground truth to every metric) is accepted and ignored: NIQE needs no reference image."""
    mu, cov = load_pris_params(pris_params)
    return float(niqe_from_stats(niqe_block_stats(img, crop_border, input_order), mu, cov).mean())


class NiqeSums:
    """Device-side NIQE of a whole dataset, in the style of ``MetricSums``: ``add(img)`` takes a (B, C, H, W) fp32 device tensor in [0, 1],
    launches the kernels (dcpt_amd.functional.niqe_stats, no host synchronisation) and keeps the [P][nblk][2][5][6] sums on the device;
    ``result()`` copies everything to the host in ONE transfer, runs the finish and returns ``{"niqe": [...]}``, one value per ``add``."""

    def __init__(self, crop_border=0, input_order="BCHW", convert_to="y", pris_params=None, **kwargs):
        if input_order != "BCHW":
            raise ValueError(f"calculate_niqe takes BCHW images only (input_order {input_order!r})")
        self.crop_border = int(crop_border)
        self._pris = load_pris_params(pris_params)
        self._parts = []

    def add(self, img, img2=None):
        from dcpt_amd import functional as DF

        _geometry(img.shape, self.crop_border, "BCHW")
        self._parts.append(DF.niqe_stats(img, self.crop_border))

    def pending(self):
        """the device tensors ``result`` needs, flat, as 8-byte words (``MetricSums.pending``)"""
        import torch

        return [t.reshape(-1).view(torch.int64) for t in self._parts]

    def result(self, host=None):
        """``host``: the int64 numpy array of ``torch.cat(self.pending())`` if the caller made the transfer; else it is made here"""
        import torch

        out = {"niqe": []}
        if not self._parts:
            return out
        if host is None:
            host = torch.cat(self.pending()).cpu().numpy()   # the one transfer
        host = host.view(np.float64)
        pos = 0
        for t in self._parts:
            stats = host[pos:pos + t.numel()].reshape(tuple(t.shape))
            pos += t.numel()
            out["niqe"].append(float(niqe_from_stats(stats, *self._pris).mean()))
        return out


def calculate_niqe_device(img, crop_border, input_order="BCHW", convert_to="y", pris_params=None, **kwargs):
    """``calculate_niqe`` for a (B, C, H, W) fp32 tensor on the device; returns a Python float (this call synchronises)"""
    acc = NiqeSums(crop_border, input_order, convert_to, pris_params)
    acc.add(img)
    return acc.result()["niqe"][0]
