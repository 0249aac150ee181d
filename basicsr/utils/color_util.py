"""Colour conversions on tensors (reference basicsr/utils/color_util.py).  Only what the metrics need: ``rgb2ycbcr_pt``."""
import torch

_YCBCR = ((65.481, -37.797, 112.0), (128.553, -74.203, -93.786), (24.966, 112.0, -18.214))   # BT.601, rows R, G, B
_OFFSET = (16.0, 128.0, 128.0)


def rgb2ycbcr_pt(img, y_only=False):
    """the reference's ``rgb2ycbcr_pt`` (color_util.py:222-254): (n, 3, h, w) RGB in [0, 1] -> (n, 3 / 1, h, w) YCbCr / Y in [0, 1], ITU-R
    BT.601.  As there, the channel mix is a matmul over the channel axis in the dtype and on the device of ``img`` (the order of its three
    products and sums is torch's), then the offset is added and the result divided by 255."""
    cols = slice(0, 1) if y_only else slice(0, 3)
    weight = torch.tensor(_YCBCR)[:, cols].contiguous().to(img)
    offset = torch.tensor(_OFFSET[cols]).view(1, -1, 1, 1).to(img)
    mixed = torch.matmul(img.permute(0, 2, 3, 1), weight).permute(0, 3, 1, 2)
    return ((mixed + 16.0) if y_only else (mixed + offset)) / 255.0
