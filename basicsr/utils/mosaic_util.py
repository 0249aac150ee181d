"""The Bayer helpers of the reference's basicsr/utils/mosaic_util.py under the same names: the RGGB masks and the mosaic on the host
(numpy), and the two demosaics ``dm`` (bilinear, circular padding) and ``dm_matlab`` (Malvar-He-Cutler, reflect padding) as thin callers
of dcpt_amd.functional.demosaic -- one fused HIP kernel of dcpt_amd/csrc/degrade.hip; there is no torch fallback.  Forward only."""
import numpy as np

__all__ = ["masks_CFA_Bayer", "mosaic_CFA_Bayer", "dm", "dm_matlab"]


def masks_CFA_Bayer(shape):
    """boolean (H, W) masks of the R, G and B sites of an RGGB array: R at (even row, even column), B at (odd, odd), G elsewhere"""
    rows, cols = np.indices(tuple(shape[:2])) % 2
    r, b = (rows == 0) & (cols == 0), (rows == 1) & (cols == 1)
    return r, ~(r | b), b


def mosaic_CFA_Bayer(RGB):
    """(CFA, CFA4, mosaic, mask) of an (H, W, 3) image with even H and W: the uint8 CFA plane, its four phases (H / 2, W / 2, 4) in the order
    (0, 0), (0, 1), (1, 0), (1, 1), the image with every sample the sensor does not see zeroed, and the (H, W, 3) boolean site mask"""
    RGB = np.asarray(RGB)
    h, w = RGB.shape[:2]
    if h % 2 or w % 2:
        raise ValueError(f"mosaic_CFA_Bayer packs 2 x 2 phases: H and W must be even, got {(h, w)} (demosaic itself takes odd sizes)")
    mask = np.stack(masks_CFA_Bayer((h, w)), axis=-1)
    mosaic = mask * RGB
    CFA = mosaic.sum(2).astype(np.uint8)
    CFA4 = np.stack([CFA[0::2, 0::2], CFA[0::2, 1::2], CFA[1::2, 0::2], CFA[1::2, 1::2]], axis=-1)
    return CFA, CFA4, mosaic, mask


def _interleave(imgs):
    """(N, 4, H / 2, W / 2) phases -> the (N, 1, H, W) CFA plane"""
    if imgs.dim() != 4 or imgs.shape[1] != 4:
        raise ValueError(f"expected the (N, 4, H / 2, W / 2) pack of the four CFA phases, got {tuple(imgs.shape)}")
    n, _, h, w = imgs.shape
    cfa = imgs.new_empty((n, 1, 2 * h, 2 * w))
    for k in range(4):
        cfa[:, 0, k // 2::2, k % 2::2] = imgs[:, k]
    return cfa


def _demosaic(imgs, method):
    from dcpt_amd import functional as DF

    return DF.demosaic(_interleave(imgs), method=method)   # (a CPU tensor raises there: no CPU fallback)


def dm(imgs):
    """bilinear demosaic of the (N, 4, H / 2, W / 2) pack: (N, 3, H, W)"""
    return _demosaic(imgs, "bilinear")


def dm_matlab(imgs):
    """Malvar-He-Cutler demosaic (MATLAB's ``demosaic``) of the (N, 4, H / 2, W / 2) pack: (N, 3, H, W)"""
    return _demosaic(imgs, "malvar")
