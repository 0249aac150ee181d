"""The LDL artifact map of the reference's basicsr/losses/loss_util.py:100-165, under the reference's import line
``from basicsr.losses.loss_util import get_refined_artifact_map``.  Of the reference's function only the path its SRModel reaches is a real
one -- ``std=True``, ``ksize=7``, no ``img_ema`` -- and that path runs on the fused fp64 kernels of dcpt_amd/csrc/ldl.hip
(dcpt_amd.functional.ldl_weight); there is no torch fallback."""

__all__ = ["get_refined_artifact_map"]


def get_refined_artifact_map(img_gt, img_output, img_ema=None, ksize=7, std=False):
    """the weight of each pixel as an artifact pixel, (B, C, H, W) fp32: w = (tanh((u - mean u) / std u) + 1) / 2 with u the unbiased
    standard deviation of |img_gt - img_output| over the reflect-padded 7 x 7 window around the pixel.  Differentiable with respect to
    ``img_output``, as in the reference, which does not detach the map."""
    if not std:
        raise NotImplementedError("get_refined_artifact_map(std=False): the reference's own std=False path needs an img_ema that SRModel "
                                  "never passes (without one it reads an unbound residual_ema); only std=True is built")
    if ksize != 7:   # (``img_ema`` is not read with std=True, here as in the reference)
        raise NotImplementedError(f"get_refined_artifact_map: the window is 7 and nothing else (got ksize={ksize})")
    from dcpt_amd import functional as DF

    return DF.ldl_weight(img_gt, img_output)
