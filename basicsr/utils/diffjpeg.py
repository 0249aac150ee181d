"""The batch JPEG codec of the reference's basicsr/utils/diffjpeg.py under the reference's import line
``from basicsr.utils import DiffJPEG``: the reference's constructor and ``forward(x, quality)``, plus ``quality_to_factor``.  The module is
a thin caller of dcpt_amd.functional.diffjpeg: the whole round trip (colour transform, chroma subsampling, 8 x 8 DCT, quantisation with the
standard luma / chroma tables, rounding, and the way back) is one fused fp64 kernel of dcpt_amd/csrc/jpeg.hip, which holds the tables as
data; there is no torch fallback.  Forward only: ``differentiable=True`` selects the cubic rounding ``round(t) + (t - round(t))^3`` in the
forward, and an input that requires grad is refused under grad mode.  One departure from the reference: a quality tensor is read, not
overwritten with the factors."""
from torch import nn

__all__ = ["DiffJPEG", "quality_to_factor"]


def quality_to_factor(quality):
    """the factor the quantisation tables are multiplied by: 50 / quality below 50, 2 - quality / 50 from 50 on"""
    scaled = 5000.0 / quality if quality < 50 else 200.0 - quality * 2
    return scaled / 100.0


class DiffJPEG(nn.Module):
    """JPEG compression and decompression of a batch; the result differs slightly from cv2's.

    Args:
        differentiable (bool): the cubic rounding function instead of ``torch.round``.
    """

    def __init__(self, differentiable=True):
        super().__init__()
        self.differentiable = bool(differentiable)

    def forward(self, x, quality):
        """x: (B, 1 or 3, H, W) RGB batch in [0, 1] on the device; quality: a number in (0, 100) or a (B,) tensor"""
        from dcpt_amd import functional as DF

        return DF.diffjpeg(x, quality, differentiable=self.differentiable)
