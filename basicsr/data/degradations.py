"""The Gaussian-noise family of the reference's basicsr/data/degradations.py (:530-634) on the fused Philox kernel
(``dcpt_amd.functional.gaussian_noise``, include/dcpt_hip.h dcpt_gauss_noise_fwd): the reference's names and signatures plus one trailing
keyword ``key=None``.  ``img`` is a (b, c, h, w) float32 device tensor; each call is ONE kernel launch for the batch.  (The Poisson family
follows further down.)

``key``: the 64-bit key of image 0's noise stream; image ``b`` uses ``key + b``.  With ``key=None`` a 63-bit base is drawn from torch's
default CPU generator, so ``torch.manual_seed`` governs the noise.  ``sigma`` and ``gray_noise`` take a number or a per-image tensor, as
in the reference.  ``random_*`` draw sigma and the gray decision per image with ``torch.rand`` on that host generator (first the b
sigmas, then the b gray draws, then the key), so nothing is read back from the device.

Departures from the reference:
  * the stream is Philox4x32-10 with Box-Muller in fp64, not torch's ``randn``: results match the reference's in distribution, not in
    value; the sum ``img + noise`` is taken in fp64 and rounded once;
  * gray noise is independent per image.  The reference's ``randn(h, w).view(b, 1, h, w)`` only works for ``b == 1``;
  * ``rounds`` rounds half to even on ``255 v`` like ``torch.round``; with ``clip`` the clamp comes first, which gives the same value as
    the reference's ``clamp(round(255 v), 0, 255) / 255``.

The blur-kernel generators of the reference (:17-479) are here too, on the host in numpy float64 with the reference's names, argument
lists and defaults: ``sigma_matrix2``, ``mesh_grid``, ``pdf2``, ``cdf2``, ``bivariate_Gaussian``, ``bivariate_generalized_Gaussian``,
``bivariate_plateau``, their ``random_*`` forms, ``random_mixed_kernels`` and ``circular_lowpass_kernel``.  They make the same draws from
``random`` and ``np.random`` in the same order as the reference, so a seeded call gives the reference's kernel.  One extension: every
``random_*`` function takes ``rng=None``, a pair (a ``random.Random``-like object, a ``np.random.RandomState``-like object) used in place
of the two modules.  The kernels are applied by ``basicsr.utils.filter2D`` (device; ``USMSharp`` is built on it) or
``basicsr.data.filter2d_host``.

The Poisson (shot-noise) family of the reference (:690-814) is here as well, on two fused kernels (``dcpt_amd.functional.poisson_noise``,
include/dcpt_hip.h dcpt_poisson_noise_fwd: a level-count pass and a sampler, two launches per call whatever the batch):
``generate_poisson_noise_pt``, ``add_poisson_noise_pt``, ``random_generate_poisson_noise_pt`` and ``random_add_poisson_noise_pt`` with the
reference's names, argument order and defaults plus the trailing ``key=None``; keys and the ``random_*`` draws (first the b scales, then
the b gray draws, then the key) as for the Gaussian functions.  They are public module attributes, imported by name.  Departures from
the reference:
  * the draws come from Philox4x32-10 by inversion, not from ``torch.poisson``: values match in distribution, not in value;
  * the rate and the quantised image are fp64, not fp32 (the levels are identical for inputs on the 8-bit grid);
  * a gray flag SELECTS the gray noise for its image where the reference blends ``noise (1 - g) + noise_gray g``: the same thing for
    flags in {0, 1};
  * gray noise needs 1 or 3 channels (the reference's ``rgb_to_grayscale`` refuses other counts too);
  * the sampler resolves ``u`` to 2^-32, so a count whose probability is below that is never drawn.
Batches of one kind only: a ``noise_type: poisson`` sample of PairedImageDenoiseDataset has no ``degrade_kind`` of its own, and
``basicsr.data.degrade_collate`` refuses it next to samples of another kind.

The second-order mixed degradation (Real-ESRGAN's chain of blur, resize, noise and JPEG, twice, with a final sinc filter) is at the end of
the module: ``draw_second_order_plan`` makes a batch's draws on the host, ``apply_second_order`` runs the device ops
(``dcpt_amd.functional.filter2d``, ``interpolate``, ``gaussian_noise`` / ``poisson_noise``, ``diffjpeg``).  One scale, one resize mode and
one noise kind serve the whole batch in each step; there is no training-pair pool and no host backend of the chain.

Out of scope: JPEG compression (see ``dcpt_amd.functional.diffjpeg``) and the numpy forms of the noise functions
(``generate_gaussian_noise``, ``add_gaussian_noise``, ``generate_poisson_noise``, ``add_poisson_noise``, ``random_*`` without ``_pt``)."""
import math
import random

import numpy as np
import torch

from dcpt_amd import functional as DF

# (the star-import list stays the device functions; the host-side blur-kernel generators below are public module attributes, imported by
# name as the reference's callers do)
__all__ = ["generate_gaussian_noise_pt", "add_gaussian_noise_pt", "random_generate_gaussian_noise_pt", "random_add_gaussian_noise_pt"]


# ---- blur kernels (host, numpy float64) ------------------------------------------------------------------
def sigma_matrix2(sig_x, sig_y, theta):
    """the covariance U diag(sig_x^2, sig_y^2) U^T of an axis-aligned Gaussian rotated by ``theta`` (radians)"""
    c, s = np.cos(theta), np.sin(theta)
    u = np.array([[c, -s], [s, c]])
    return np.dot(u, np.dot(np.array([[sig_x ** 2, 0], [0, sig_y ** 2]]), u.T))


def mesh_grid(kernel_size):
    """the grid centred at zero: ``xy`` (K, K, 2) with xy[i, j] = (x_j, y_i), and ``xx``, ``yy`` (K, K)"""
    ax = np.arange(-kernel_size // 2 + 1.0, kernel_size // 2 + 1.0)
    xx, yy = np.meshgrid(ax, ax)
    return np.stack((xx, yy), axis=2), xx, yy


def _quadratic_form(sigma_matrix, grid):
    """g^T Sigma^-1 g at every grid point g"""
    return np.sum(np.dot(grid, np.linalg.inv(sigma_matrix)) * grid, 2)


def pdf2(sigma_matrix, grid):
    """the un-normalised bivariate Gaussian density exp(-g^T Sigma^-1 g / 2) on the grid"""
    return np.exp(-0.5 * _quadratic_form(sigma_matrix, grid))


def cdf2(d_matrix, grid):
    """the CDF of the standard bivariate normal at ``grid @ d_matrix`` (the skew of a skewed Gaussian); needs scipy"""
    from scipy.stats import multivariate_normal

    return multivariate_normal([0, 0], [[1, 0], [0, 1]]).cdf(np.dot(grid, d_matrix))


def _sigma(sig_x, sig_y, theta, isotropic):
    return np.array([[sig_x ** 2, 0], [0, sig_x ** 2]]) if isotropic else sigma_matrix2(sig_x, sig_y, theta)


def bivariate_Gaussian(kernel_size, sig_x, sig_y, theta, grid=None, isotropic=True):
    """the normalised Gaussian kernel; ``isotropic`` uses ``sig_x`` alone"""
    if grid is None:
        grid, _, _ = mesh_grid(kernel_size)
    kernel = pdf2(_sigma(sig_x, sig_y, theta, isotropic), grid)
    return kernel / np.sum(kernel)


def bivariate_generalized_Gaussian(kernel_size, sig_x, sig_y, theta, beta, grid=None, isotropic=True):
    """the normalised generalised Gaussian exp(-(g^T Sigma^-1 g)^beta / 2); beta = 1 is the Gaussian"""
    if grid is None:
        grid, _, _ = mesh_grid(kernel_size)
    kernel = np.exp(-0.5 * np.power(_quadratic_form(_sigma(sig_x, sig_y, theta, isotropic), grid), beta))
    return kernel / np.sum(kernel)


def bivariate_plateau(kernel_size, sig_x, sig_y, theta, beta, grid=None, isotropic=True):
    """the normalised plateau kernel 1 / ((g^T Sigma^-1 g)^beta + 1)"""
    if grid is None:
        grid, _, _ = mesh_grid(kernel_size)
    kernel = np.reciprocal(np.power(_quadratic_form(_sigma(sig_x, sig_y, theta, isotropic), grid), beta) + 1)
    return kernel / np.sum(kernel)


def _generators(rng):
    return (random, np.random) if rng is None else rng


def _draw_shape(nr, kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic):
    """sigma_x, then (anisotropic only) sigma_y and the rotation, each one ``uniform`` of the numpy generator"""
    assert kernel_size % 2 == 1, "Kernel size must be an odd number."
    assert sigma_x_range[0] < sigma_x_range[1], "Wrong sigma_x_range."
    sigma_x = nr.uniform(sigma_x_range[0], sigma_x_range[1])
    if isotropic is False:
        assert sigma_y_range[0] < sigma_y_range[1], "Wrong sigma_y_range."
        assert rotation_range[0] < rotation_range[1], "Wrong rotation_range."
        return sigma_x, nr.uniform(sigma_y_range[0], sigma_y_range[1]), nr.uniform(rotation_range[0], rotation_range[1])
    return sigma_x, sigma_x, 0


def _draw_beta(nr, beta_range):
    """one draw picks the side of 1, a second the value on it (the range is taken to straddle 1)"""
    if nr.uniform() < 0.5:
        return nr.uniform(beta_range[0], 1)
    return nr.uniform(1, beta_range[1])


def _noisy(nr, kernel, noise_range):
    """multiplicative noise, one uniform draw per entry, and the final normalisation"""
    if noise_range is not None:
        assert noise_range[0] < noise_range[1], "Wrong noise range."
        kernel = kernel * nr.uniform(noise_range[0], noise_range[1], size=kernel.shape)
    return kernel / np.sum(kernel)


def random_bivariate_Gaussian(kernel_size, sigma_x_range, sigma_y_range, rotation_range, noise_range=None, isotropic=True, rng=None):
    nr = _generators(rng)[1]
    sigma_x, sigma_y, rotation = _draw_shape(nr, kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    return _noisy(nr, bivariate_Gaussian(kernel_size, sigma_x, sigma_y, rotation, isotropic=isotropic), noise_range)


def random_bivariate_generalized_Gaussian(kernel_size, sigma_x_range, sigma_y_range, rotation_range, beta_range, noise_range=None,
                                          isotropic=True, rng=None):
    nr = _generators(rng)[1]
    sigma_x, sigma_y, rotation = _draw_shape(nr, kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    beta = _draw_beta(nr, beta_range)
    return _noisy(nr, bivariate_generalized_Gaussian(kernel_size, sigma_x, sigma_y, rotation, beta, isotropic=isotropic), noise_range)


def random_bivariate_plateau(kernel_size, sigma_x_range, sigma_y_range, rotation_range, beta_range, noise_range=None, isotropic=True,
                             rng=None):
    nr = _generators(rng)[1]
    sigma_x, sigma_y, rotation = _draw_shape(nr, kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    beta = _draw_beta(nr, beta_range)
    return _noisy(nr, bivariate_plateau(kernel_size, sigma_x, sigma_y, rotation, beta, isotropic=isotropic), noise_range)


def random_mixed_kernels(kernel_list, kernel_prob, kernel_size=21, sigma_x_range=(0.6, 5), sigma_y_range=(0.6, 5),
                         rotation_range=(-math.pi, math.pi), betag_range=(0.5, 8), betap_range=(0.5, 8), noise_range=None, rng=None):
    """one kernel of a type drawn from ``kernel_list`` with the weights ``kernel_prob`` (``random.choices``): ``iso``, ``aniso``,
    ``generalized_iso``, ``generalized_aniso``, ``plateau_iso``, ``plateau_aniso``.  As in the reference the plateau kernels take no
    multiplicative noise, and an unknown type is an error here (the reference fails on the unbound result)."""
    kernel_type = _generators(rng)[0].choices(kernel_list, kernel_prob)[0]
    family, _, shape = kernel_type.rpartition("_")
    if shape not in ("iso", "aniso") or family not in ("", "generalized", "plateau"):
        raise ValueError(f"unknown kernel type {kernel_type!r}")
    common = (kernel_size, sigma_x_range, sigma_y_range, rotation_range)
    if family == "":
        return random_bivariate_Gaussian(*common, noise_range=noise_range, isotropic=shape == "iso", rng=rng)
    if family == "generalized":
        return random_bivariate_generalized_Gaussian(*common, betag_range, noise_range=noise_range, isotropic=shape == "iso", rng=rng)
    return random_bivariate_plateau(*common, betap_range, noise_range=None, isotropic=shape == "iso", rng=rng)


def circular_lowpass_kernel(cutoff, kernel_size, pad_to=0):
    """the normalised 2-D sinc (jinc) filter cutoff J1(cutoff d) / (2 pi d) at distance d from the centre, cutoff^2 / (4 pi) at it;
    ``cutoff`` in radians (pi is the maximum), ``pad_to`` an odd size to zero-pad to (0: none); needs scipy"""
    from scipy import special

    assert kernel_size % 2 == 1, "Kernel size must be an odd number."
    mid = (kernel_size - 1) / 2
    ii, jj = np.indices((kernel_size, kernel_size), dtype=float)
    d = np.sqrt((ii - mid) ** 2 + (jj - mid) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        kernel = cutoff * special.j1(cutoff * d) / (2 * np.pi * d)
    kernel[(kernel_size - 1) // 2, (kernel_size - 1) // 2] = cutoff ** 2 / (4 * np.pi)
    kernel = kernel / np.sum(kernel)
    if pad_to > kernel_size:
        pad = (pad_to - kernel_size) // 2
        kernel = np.pad(kernel, ((pad, pad), (pad, pad)))
    return kernel


# ---- Gaussian noise (device) --------------------------------------------------------------------------------


def _keys(b, key):
    if key is None:
        # 63 bits from the default CPU generator (torch.manual_seed governs it); randint's exclusive bound must itself fit int64
        hi, lo = torch.randint(0, 1 << 31, (2,), dtype=torch.int64).tolist()
        key = (hi << 32) | (lo << 1) | int(torch.randint(0, 2, (1,)).item())
    key = int(key)
    return torch.tensor([(key + i + (1 << 63)) % (1 << 64) - (1 << 63) for i in range(b)], dtype=torch.int64)   # (the low 64 bits, signed)


def _noise(img, sigma, gray_noise, key, **flags):
    if not torch.is_tensor(img) or img.dim() != 4:
        raise ValueError("expected a (b, c, h, w) tensor")
    b = img.shape[0]
    if not torch.is_tensor(gray_noise):
        gray_noise = int(gray_noise > 0)
    return DF.gaussian_noise(img, sigma, _keys(b, key), gray=gray_noise, **flags)


def _random(img, sigma_range, gray_prob):
    b = img.shape[0]
    sigma = torch.rand(b) * (sigma_range[1] - sigma_range[0]) + sigma_range[0]
    gray = (torch.rand(b) < gray_prob).int()
    return sigma, gray


def generate_gaussian_noise_pt(img, sigma=10, gray_noise=0, key=None):
    """the noise ``sigma / 255 * n`` of the shape of ``img`` (reference :530-563)"""
    return _noise(img, sigma, gray_noise, key, noise_only=True)


def add_gaussian_noise_pt(img, sigma=10, gray_noise=0, clip=True, rounds=False, key=None):
    """``img`` + Gaussian noise, clamped to [0, 1] (``clip``) and / or rounded to the 8-bit grid (``rounds``) (reference :566-585)"""
    return _noise(img, sigma, gray_noise, key, clip=clip, rounds=rounds)


def random_generate_gaussian_noise_pt(img, sigma_range=(0, 10), gray_prob=0, key=None):
    """noise with a sigma drawn uniformly from ``sigma_range`` and gray with probability ``gray_prob``, per image (reference :612-620)"""
    sigma, gray = _random(img, sigma_range, gray_prob)
    return _noise(img, sigma, gray, key, noise_only=True)


def random_add_gaussian_noise_pt(img, sigma_range=(0, 1.0), gray_prob=0, clip=True, rounds=False, key=None):
    """``img`` + that noise (reference :623-634)"""
    sigma, gray = _random(img, sigma_range, gray_prob)
    return _noise(img, sigma, gray, key, clip=clip, rounds=rounds)


# ---- Poisson noise (device) ---------------------------------------------------------------------------------


def _poisson(img, scale, gray_noise, key, **flags):
    if not torch.is_tensor(img) or img.dim() != 4:
        raise ValueError("expected a (b, c, h, w) tensor")
    b = img.shape[0]
    if not torch.is_tensor(gray_noise):
        gray_noise = int(gray_noise > 0)
    return DF.poisson_noise(img, scale, _keys(b, key), gray=gray_noise, **flags)


def generate_poisson_noise_pt(img, scale=1.0, gray_noise=0, key=None):
    """the shot noise ``scale * (Poisson(q vals) / vals - q)`` of the shape of ``img``, q the image (or its gray values) on the 8-bit grid
    and vals its level count rounded up to a power of two (reference :690-738)"""
    return _poisson(img, scale, gray_noise, key, noise_only=True)


def add_poisson_noise_pt(img, scale=1.0, clip=True, rounds=False, gray_noise=0, key=None):
    """``img`` + Poisson noise, clamped to [0, 1] (``clip``) and / or rounded to the 8-bit grid (``rounds``) (reference :741-763)"""
    return _poisson(img, scale, gray_noise, key, clip=clip, rounds=rounds)


def random_generate_poisson_noise_pt(img, scale_range=(0, 1.0), gray_prob=0, key=None):
    """noise with a scale drawn uniformly from ``scale_range`` and gray with probability ``gray_prob``, per image (reference :792-800)"""
    scale, gray = _random(img, scale_range, gray_prob)
    return _poisson(img, scale, gray, key, noise_only=True)


def random_add_poisson_noise_pt(img, scale_range=(0, 1.0), gray_prob=0, clip=True, rounds=False, key=None):
    """``img`` + that noise (reference :803-814)"""
    scale, gray = _random(img, scale_range, gray_prob)
    return _poisson(img, scale, gray, key, clip=clip, rounds=rounds)


# ---- the second-order mixed degradation (device) --------------------------------------------------------------
# The chain this toolbox exists for (Real-ESRGAN, Wang et al., ICCVW 2021): blur -> resize -> noise -> JPEG, the same again, then a sinc filter
# and a last JPEG in either order.  Two halves: ``draw_second_order_plan`` makes every random draw of a batch on the host,
# ``apply_second_order`` runs the device ops of a plan and takes no device value in Python.  One scale, one resize mode and one noise kind
# serve a whole batch per step; sigma / scale, the gray decision and the JPEG quality are per image.
RESIZE_MODES = ("area", "bilinear", "bicubic")
SECOND_ORDER_KERNEL = 21   # the size the data set pads kernel1, kernel2 and sinc_kernel to


def _draw_resize(pr, nr, prob, scale_range):
    """the direction by ``random.choices``, the scale by one ``uniform`` (none for keep), the mode by ``random.choice``"""
    direction = pr.choices(["up", "down", "keep"], prob)[0]
    if direction == "up":
        s = float(nr.uniform(1, scale_range[1]))
    elif direction == "down":
        s = float(nr.uniform(scale_range[0], 1))
    else:
        s = 1.0
    return s, pr.choice(RESIZE_MODES)


def _draw_noise(pr, nr, B, opt, sfx):
    """one ``uniform`` picks the kind for the batch; then B amplitudes, B gray draws and the base of the B keys"""
    gaussian = bool(nr.uniform() < opt.get("gaussian_noise_prob" + sfx, opt["gaussian_noise_prob"]))
    lo, hi = opt["noise_range" + sfx] if gaussian else opt["poisson_scale_range" + sfx]
    amp = torch.as_tensor(np.asarray(nr.uniform(lo, hi, size=B)), dtype=torch.float32)
    gray = torch.as_tensor(np.asarray(nr.uniform(size=B)) < opt["gray_noise_prob" + sfx], dtype=torch.int32)
    return {"kind": "gaussian" if gaussian else "poisson", "amp": amp, "gray": gray, "key": _keys(B, pr.getrandbits(63))}


def _draw_quality(nr, B, jpeg_range):
    return torch.as_tensor(np.asarray(nr.uniform(jpeg_range[0], jpeg_range[1], size=B)), dtype=torch.float32)


def draw_second_order_plan(opt, B, H, W, scale, rng=None):
    """Every draw of one batch of the chain, on the host: from ``(random, np.random)`` or the pair ``rng`` (the blur generators'
    convention), in the order of the steps of ``apply_second_order``.  ``opt``: ``resize_prob`` (up, down, keep), ``resize_range``,
    ``gaussian_noise_prob``, ``noise_range``, ``poisson_scale_range``, ``gray_noise_prob``, ``jpeg_range``, ``second_blur_prob`` and the
    ``*2`` forms of the first-order ones (``gaussian_noise_prob2`` defaults to ``gaussian_noise_prob``).  Returns a plain dict of host
    numbers and host tensors:
    ``resize1`` {scale_factor, mode}; ``noise1`` / ``noise2`` {kind, amp (B,) fp32, gray (B,) int32, key (B,) int64, made by ``_keys``
    from 63 bits of the Python generator}; ``jpeg1`` / ``jpeg2`` (B,) fp32 qualities; ``second_blur``; ``resize2`` {size, mode} with
    size ``(int(H / scale * s), int(W / scale * s))``; ``final_first`` (the resize-and-sinc step before the last JPEG); ``final_mode``;
    ``out_size`` ``(H // scale, W // scale)``.
    Raises when the smallest size the options allow breaks a blur's reflect padding (``K // 2`` below every H and W it meets, K = 21)."""
    pr, nr = _generators(rng)
    r = SECOND_ORDER_KERNEL // 2
    least1 = math.floor(min(H, W) * (opt["resize_range"][0] if opt["resize_prob"][1] > 0 else 1.0))
    for what, side in (("gt", min(H, W)), ("the first resize's smallest output", least1), ("lq", min(H, W) // scale)):
        if side <= r:
            raise ValueError(f"second-order degradation: {what} can be {side} pixels on a side, which the reflect padding {r} of a "
                             f"{SECOND_ORDER_KERNEL} x {SECOND_ORDER_KERNEL} blur does not fit (gt {H} x {W}, scale {scale}, "
                             f"resize_range {list(opt['resize_range'])})")
    if min(int(H / scale * opt["resize_range2"][0]), int(W / scale * opt["resize_range2"][0])) < 1 and opt["resize_prob2"][1] > 0:
        raise ValueError(f"second-order degradation: resize_range2 {list(opt['resize_range2'])} can give an empty image")
    plan = {"scale": scale, "gt_size": (H, W), "out_size": (H // scale, W // scale)}
    s, mode = _draw_resize(pr, nr, opt["resize_prob"], opt["resize_range"])
    plan["resize1"] = {"scale_factor": s, "mode": mode}
    plan["noise1"] = _draw_noise(pr, nr, B, opt, "")
    plan["jpeg1"] = _draw_quality(nr, B, opt["jpeg_range"])
    plan["second_blur"] = bool(nr.uniform() < opt["second_blur_prob"])
    s, mode = _draw_resize(pr, nr, opt["resize_prob2"], opt["resize_range2"])
    plan["resize2"] = {"scale_factor": s, "size": (int(H / scale * s), int(W / scale * s)), "mode": mode}
    plan["noise2"] = _draw_noise(pr, nr, B, opt, "2")
    plan["final_first"] = bool(nr.uniform() < 0.5)
    plan["final_mode"] = pr.choice(RESIZE_MODES)
    plan["jpeg2"] = _draw_quality(nr, B, opt["jpeg_range2"])
    return plan


def second_order_steps(gt, kernel1, kernel2, sinc_kernel, plan):
    """the chain step by step: yields ``(name, tensor)`` after every device op, the last one ``("lq", lq)``"""
    def noise(out, n):
        op = DF.gaussian_noise if n["kind"] == "gaussian" else DF.poisson_noise
        return op(out, n["amp"], n["key"], gray=n["gray"], clip=True)

    def final(out):
        out = DF.interpolate(out, size=plan["out_size"], mode=plan["final_mode"])
        return DF.filter2d(out, sinc_kernel)

    out = DF.filter2d(gt, kernel1)
    yield "blur1", out
    out = DF.interpolate(out, scale_factor=plan["resize1"]["scale_factor"], mode=plan["resize1"]["mode"])
    yield "resize1", out
    out = noise(out, plan["noise1"])   # (clipped: the JPEG's input lies in [0, 1])
    yield "noise1", out
    out = DF.diffjpeg(out, plan["jpeg1"], differentiable=False, uint8_io=False)
    yield "jpeg1", out
    if plan["second_blur"]:
        out = DF.filter2d(out, kernel2)
        yield "blur2", out
    out = DF.interpolate(out, size=plan["resize2"]["size"], mode=plan["resize2"]["mode"])
    yield "resize2", out
    out = noise(out, plan["noise2"])
    yield "noise2", out
    if plan["final_first"]:
        out = final(out)
        yield "final", out
        out = DF.diffjpeg(out.clamp(0, 1), plan["jpeg2"], differentiable=False, uint8_io=False)
        yield "jpeg2", out
    else:
        out = DF.diffjpeg(out, plan["jpeg2"], differentiable=False, uint8_io=False)
        yield "jpeg2", out
        out = final(out)
        yield "final", out
    # the last op is the sinc filter or the JPEG, never the resize, so the 8-bit grid is taken with torch expressions (half to even)
    yield "lq", torch.round(out.clamp(0, 1) * 255) / 255


def apply_second_order(gt, kernel1, kernel2, sinc_kernel, plan):
    """The second-order degradation of a batch: ``gt`` (B, 1 or 3, H, W) fp32 device tensor in [0, 1]; ``kernel1``, ``kernel2``,
    ``sinc_kernel`` (B, K, K) float tensors on any device; ``plan`` from ``draw_second_order_plan``.  Steps: ``filter2d(kernel1)``;
    ``interpolate(scale_factor)``; Gaussian or Poisson noise, clipped; ``diffjpeg``; ``filter2d(kernel2)`` where the plan says so;
    ``interpolate(size)``; noise; then the final resize to ``(H // scale, W // scale)`` with ``filter2d(sinc_kernel)`` and the last
    ``diffjpeg``, in the plan's order; ``lq = round(clamp(out, 0, 1) * 255) / 255``.  Device ops only: nothing is read back."""
    for _, out in second_order_steps(gt, kernel1, kernel2, sinc_kernel, plan):
        pass
    return out
