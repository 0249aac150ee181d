"""The Gaussian-noise family of the reference's basicsr/data/degradations.py (:530-634) on the fused Philox kernel
(``dcpt_amd.functional.gaussian_noise``, include/dcpt_hip.h dcpt_gauss_noise_fwd): the reference's names and signatures plus one trailing
keyword ``key=None``.  ``img`` is a (b, c, h, w) float32 device tensor; each call is ONE kernel launch for the batch.

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

Out of scope: the Poisson family, the blur-kernel generators (``bivariate_*``, ``random_mixed_kernels``, ``circular_lowpass_kernel``),
``filter2D`` / ``USMSharp``, JPEG compression (see ``dcpt_amd.functional.diffjpeg``) and the numpy forms (``generate_gaussian_noise``,
``add_gaussian_noise``, ``random_*`` without ``_pt``)."""
import torch

from dcpt_amd import functional as DF

__all__ = ["generate_gaussian_noise_pt", "add_gaussian_noise_pt", "random_generate_gaussian_noise_pt", "random_add_gaussian_noise_pt"]


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
