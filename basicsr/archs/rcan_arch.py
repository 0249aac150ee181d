"""RCAN, MI355X-native.

Registry name ``RCAN``, constructor kwargs, ``forward(x)`` and ``state_dict`` keys / shapes as the reference's
basicsr/archs/rcan_arch.py (``conv_first``, ``body.{g}.residual_group.{b}.rcab.{0,2}``, ``body.{g}.residual_group.{b}.rcab.3.attention.{1,3}``,
``body.{g}.conv``, ``conv_after_body``, ``upsample.{0,2,...}``, ``conv_last``).  ``mean`` is a plain attribute, not a buffer, as there.

Every RCAB is one autograd node (``dcpt_rcab_*``: conv1 + bias + ReLU, conv2 + bias with the channel-attention pooling in its epilogue,
the CA FCs, ``x + res_scale * t * s``); every group conv and ``conv_after_body`` is ``dcpt_conv3x3_res_*`` with the skip as its residual;
every Upsample stage is ``dcpt_conv3x3_ps_*`` (3 x 3 conv + PixelShuffle(r) in one GEMM).  Feature maps are channels_last.  Child modules
only own the parameters.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from basicsr.utils.registry import ARCH_REGISTRY
from dcpt_amd import functional as DF


class ChannelAttention(nn.Module):
    def __init__(self, num_feat, squeeze_factor=16):
        super().__init__()
        self.attention = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            nn.Conv2d(num_feat, num_feat // squeeze_factor, 1, padding=0),
            nn.ReLU(inplace=True),
            nn.Conv2d(num_feat // squeeze_factor, num_feat, 1, padding=0),
            nn.Sigmoid(),
        )


class RCAB(nn.Module):
    def __init__(self, num_feat, squeeze_factor=16, res_scale=1):
        super().__init__()
        self.res_scale = res_scale
        self.rcab = nn.Sequential(
            nn.Conv2d(num_feat, num_feat, 3, 1, 1),
            nn.ReLU(True),
            nn.Conv2d(num_feat, num_feat, 3, 1, 1),
            ChannelAttention(num_feat, squeeze_factor),
        )

    def forward(self, x):
        c1, c2, att = self.rcab[0], self.rcab[2], self.rcab[3].attention
        return DF.rcab(x, c1.weight, c1.bias, c2.weight, c2.bias, att[1].weight, att[1].bias, att[3].weight, att[3].bias, self.res_scale)


class ResidualGroup(nn.Module):
    def __init__(self, num_feat, num_block, squeeze_factor=16, res_scale=1):
        super().__init__()
        self.residual_group = nn.Sequential(
            *[RCAB(num_feat=num_feat, squeeze_factor=squeeze_factor, res_scale=res_scale) for _ in range(num_block)])
        self.conv = nn.Conv2d(num_feat, num_feat, 3, 1, 1)

    def forward(self, x):
        t = x
        for blk in self.residual_group:
            t = blk(t)
        return DF.conv3x3_res(t, self.conv.weight, self.conv.bias, x)


class Upsample(nn.Sequential):
    """arch_util.py Upsample: (Conv2d(C, 4C, 3) + PixelShuffle(2)) x log2(scale), or Conv2d(C, 9C, 3) + PixelShuffle(3)."""

    def __init__(self, scale, num_feat):
        m = []
        if (scale & (scale - 1)) == 0:  # scale = 2^n
            for _ in range(int(math.log(scale, 2))):
                m.append(nn.Conv2d(num_feat, 4 * num_feat, 3, 1, 1))
                m.append(nn.PixelShuffle(2))
        elif scale == 3:
            m.append(nn.Conv2d(num_feat, 9 * num_feat, 3, 1, 1))
            m.append(nn.PixelShuffle(3))
        else:
            raise ValueError(f"scale {scale} is not supported. Supported scales: 2^n and 3.")
        super().__init__(*m)

    def forward(self, x):
        mods = list(self)
        for conv, shuffle in zip(mods[0::2], mods[1::2]):
            x = DF.conv3x3_ps(x, conv.weight, conv.bias, shuffle.upscale_factor)
        return x


@ARCH_REGISTRY.register()
class RCAN(nn.Module):
    def __init__(self, num_in_ch, num_out_ch, num_feat=64, num_group=10, num_block=16, squeeze_factor=16, upscale=4, res_scale=1,
                 img_range=255.0, rgb_mean=(0.4488, 0.4371, 0.4040)):
        super().__init__()
        if num_feat % 4:
            raise NotImplementedError(f"num_feat={num_feat}: the RCAN kernels need a multiple of 4 channels")
        if num_feat // squeeze_factor < 1:
            raise NotImplementedError(f"num_feat={num_feat}, squeeze_factor={squeeze_factor}: the channel attention needs num_feat // squeeze_factor >= 1")
        self.img_range = img_range
        self.mean = torch.Tensor(rgb_mean).view(1, 3, 1, 1)
        self.conv_first = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[
            ResidualGroup(num_feat=num_feat, num_block=num_block, squeeze_factor=squeeze_factor, res_scale=res_scale)
            for _ in range(num_group)])
        self.conv_after_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.upsample = Upsample(upscale, num_feat)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)

    def forward(self, x):
        self.mean = self.mean.type_as(x)
        cin = x.shape[1]
        mean = self.mean.reshape(-1)
        if mean.numel() != cin:
            raise ValueError(f"RCAN: rgb_mean has {mean.numel()} entries for a {cin}-channel input")
        xn = DF.img_affine(x, mean, self.img_range, 0)
        x_first = DF.conv3x3_in(xn, self.conv_first.weight, self.conv_first.bias)
        t = x_first
        for group in self.body:
            t = group(t)
        res = DF.conv3x3_res(t, self.conv_after_body.weight, self.conv_after_body.bias, x_first)
        out = DF.conv3x3_out(self.upsample(res), self.conv_last.weight, self.conv_last.bias)
        return DF.img_affine(out, mean, self.img_range, 1)
