"""A kernel-blind restatement, in torch float64 on the CPU, of the JPEG round trip of the reference's DiffJPEG.forward
(basicsr/utils/diffjpeg.py:494-523) -- the yardstick of tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py.  Not a test.  It is written from
the formulas and knows nothing of macroblocks per workgroup, lanes or LDS:

    pad bottom / right with zeros to a multiple of 16;  v = 255 x  (uint8_io: v = round(255 x), half to even)
    Y = .299 R + .587 G + .114 B,  Cb = -.168736 R - .331264 G + .5 B + 128,  Cr = .5 R - .418688 G - .081312 B + 128
    Cb, Cr: mean over 2 x 2
    per 8 x 8 block s:  F = (a a^T / 4) * (K (s - 128) K^T),  K[k][n] = cos((2n + 1) k pi / 16), a = (1 / sqrt 2, 1, .., 1)
    t = F / (table * factor):  table the transposed luma table for Y, the chroma table for Cb / Cr;
        factor = (5000 / q if q < 50 else 200 - 2 q) / 100, per image
    r = round(t) (half to even)   or, differentiable,   r = round(t) + (t - round(t))^3
    D = r * table * factor;  s' = K^T ((a a^T) * D) K / 4 + 128
    chroma repeated 2 x 2;  R = Y + 1.402 (Cr - 128), G = Y - .344136 (Cb - 128) - .714136 (Cr - 128), B = Y + 1.772 (Cb - 128)
    clamp to [0, 255], / 255, crop to H x W  (uint8_io: round(clamped) / 255)
    one-channel input: the plane is all three channels; the output is the mean of the three decoded channels
    (uint8_io: round(mean of the three clamped channels) / 255)

``diffjpeg`` returns the output together with every pre-round value t (for the tie census of the GPU test) and, for ``uint8_io``, the
pre-round output in 0..255 units."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

LUMA = torch.tensor([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                     [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                     [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], dtype=torch.float64).t().contiguous()
CHROMA = torch.full((8, 8), 99.0, dtype=torch.float64)
CHROMA[:4, :4] = torch.tensor([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]], dtype=torch.float64).t()
K = torch.tensor([[math.cos((2 * n + 1) * k * math.pi / 16) for n in range(8)] for k in range(8)], dtype=torch.float64)
ALPHA = torch.tensor([1 / math.sqrt(2)] + [1.0] * 7, dtype=torch.float64)
AA = torch.outer(ALPHA, ALPHA)

Result = namedtuple("Result", "y t_y t_cb t_cr pre")   # t_*: (B, block rows, block columns, 8, 8); pre: (B, C, H, W) in 0..255 or None


def quality_to_factor(q):
    q = torch.as_tensor(q, dtype=torch.float64)
    return torch.where(q < 50, 5000.0 / q, 200.0 - 2.0 * q) / 100.0


def _blocks(p):
    B, h, w = p.shape
    return p.reshape(B, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4)


def _merge(b):
    B, nh, nw, _, _ = b.shape
    return b.permute(0, 1, 3, 2, 4).reshape(B, nh * 8, nw * 8)


def _codec(plane, table, factor, differentiable):
    s = _blocks(plane) - 128.0
    f = (AA / 4) * (K @ s @ K.t())
    div = table * factor.view(-1, 1, 1, 1, 1)
    t = f / div
    r = torch.round(t)
    if differentiable:
        r = r + (t - r) ** 3
    d = r * div
    return _merge(K.t() @ (AA * d) @ K / 4 + 128.0), t


def diffjpeg(x, quality, differentiable=False, uint8_io=False):
    x = x.detach().cpu().double()
    B, C, H, W = x.shape
    assert C in (1, 3)
    if torch.is_tensor(quality):
        q = quality.detach().cpu().double().reshape(B)
    else:
        q = torch.full((B,), float(quality), dtype=torch.float64)
    factor = quality_to_factor(q)
    if C == 1:
        x = x.repeat(1, 3, 1, 1)
    v = F.pad(x, (0, -W % 16, 0, -H % 16)) * 255.0
    if uint8_io:
        v = torch.round(v)
    r, g, b = v[:, 0], v[:, 1], v[:, 2]
    Y = 0.299 * r + 0.587 * g + 0.114 * b
    cb = -0.168736 * r - 0.331264 * g + 0.5 * b + 128.0
    cr = 0.5 * r - 0.418688 * g - 0.081312 * b + 128.0
    cb, cr = F.avg_pool2d(cb.unsqueeze(1), 2).squeeze(1), F.avg_pool2d(cr.unsqueeze(1), 2).squeeze(1)
    Y, t_y = _codec(Y, LUMA, factor, differentiable)
    cb, t_cb = _codec(cb, CHROMA, factor, differentiable)
    cr, t_cr = _codec(cr, CHROMA, factor, differentiable)
    cb = cb.repeat_interleave(2, 1).repeat_interleave(2, 2) - 128.0
    cr = cr.repeat_interleave(2, 1).repeat_interleave(2, 2) - 128.0
    rgb = torch.stack([Y + 1.402 * cr, Y - 0.344136 * cb - 0.714136 * cr, Y + 1.772 * cb], 1).clamp(0.0, 255.0)[:, :, :H, :W]
    if C == 1:
        pre = rgb.mean(1, keepdim=True)
        y = torch.round(pre) / 255.0 if uint8_io else (rgb / 255.0).mean(1, keepdim=True)
    else:
        pre = rgb
        y = torch.round(pre) / 255.0 if uint8_io else rgb / 255.0
    return Result(y, t_y, t_cb, t_cr, pre if uint8_io else None)


def tie_distance(t):
    """distance of every pre-round value to the nearest rounding tie k + 1/2"""
    return ((t - torch.floor(t)) - 0.5).abs()


def tie_macroblocks(res, eps=1e-6):
    """the (image, macroblock row, macroblock column) triples that hold a coefficient within ``eps`` of a rounding tie"""
    out = set()
    for t, per in ((res.t_y, 2), (res.t_cb, 1), (res.t_cr, 1)):   # two Y blocks per macroblock edge, one chroma block
        near = (tie_distance(t) < eps).flatten(3).any(3)
        out.update((int(b), int(i) // per, int(j) // per) for b, i, j in near.nonzero().tolist())
    return sorted(out)


def macroblock_mask(shape, blocks):
    """(B, 1, H, W) bool mask of the pixels of the listed macroblocks"""
    B, _, H, W = shape
    m = torch.zeros((B, 1, H, W), dtype=torch.bool)
    for b, i, j in blocks:
        m[b, :, 16 * i:16 * i + 16, 16 * j:16 * j + 16] = True
    return m
