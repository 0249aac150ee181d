"""RCAN, MI355X-native.

Registry name ``RCAN``, constructor kwargs, ``forward(x)`` and ``state_dict`` keys / shapes as the reference's
basicsr/archs/rcan_arch.py (``conv_first``, ``body.{g}.residual_group.{b}.rcab.{0,2}``, ``body.{g}.residual_group.{b}.rcab.3.attention.{1,3}``,
``body.{g}.conv``, ``conv_after_body``, ``upsample.{0,2,...}``, ``conv_last``).  ``mean`` is a plain attribute, not a buffer, as there.

Every RCAB is one autograd node (``dcpt_rcab_*``: conv1 + bias + ReLU, conv2 + bias with the channel-attention pooling in its epilogue,
the CA FCs, ``x + res_scale * t * s``); every group conv and ``conv_after_body`` is ``dcpt_conv3x3_res_*`` with the skip as its residual;
every Upsample stage is ``dcpt_conv3x3_ps_*`` (3 x 3 conv + PixelShuffle(r) in one GEMM).  Feature maps are channels_last.  Child modules
only own the parameters.

``act_dtype="bf16"`` (this repo's extension, default "fp32"; ``network_g.act_dtype`` in the options, ``set_act_dtype`` on an existing network):
INFERENCE on bf16 activation storage.  ``conv_first`` emits a bf16 map, every RCAB (``dcpt_rcab_fwd_bf16``), group conv / ``conv_after_body``
(``dcpt_conv3x3_res_fwd_bf16``) and Upsample stage (``dcpt_conv3x3_ps_fwd_bf16``) reads and writes bf16 maps, ``conv_last`` takes the bf16 map
to the fp32 image: no fp32 feature map of the network's width exists.  Parameters, accumulation, the pooled mean, the CA FCs and the sigmoid
stay fp32.  There is no backward pass: a bf16 forward that would have to record one raises ``NotImplementedError``.  The bf16 operand images
of the 3 x 3 weights are cached per conv (``DF.PackedConvBf16``) and the stale ones refreshed in one call at the top of the forward.

``act_dtype="bf16_res32"``: the same inference path with the RESIDUAL STREAM -- the map that runs through the 160 RCAB adds and the group
convs -- kept in fp32 next to its bf16 image (``DF.Stream32``): ``conv_first`` emits fp32, every RCAB is ``dcpt_rcab_fwd_bf16_res32``, the group
convs and ``conv_after_body`` are ``dcpt_conv3x3_res_fwd_bf16_res32`` (the latter writes only the bf16 map: the stream ends there).  Every conv
operand is still bf16, h and t are bf16; only the stream's own rounding is gone.  Same restrictions, same parameters, same cached packs.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from basicsr.utils.registry import ARCH_REGISTRY
from dcpt_amd import functional as DF


_ACT_DTYPES = ("fp32", "bf16", "bf16_res32")
_BF16_MODES = ("bf16", "bf16_res32")   # inference on bf16 maps; the second keeps the residual stream in fp32


def _pack_of(conv):
    """the conv's cache of its bf16 operand images (a plain attribute: not part of the state_dict); None for a conv wider than the cached
    form takes (its entry point then packs in the call)"""
    if conv.out_channels > 1024:
        return None
    if getattr(conv, "_packed_bf16", None) is None:
        conv._packed_bf16 = DF.PackedConvBf16()
    return conv._packed_bf16


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
        if isinstance(x, DF.Stream32):   # bf16 maps around the fp32 residual stream
            return DF.Stream32(*DF.rcab_bf16_res32(x.s, x.sb, c1.weight, c1.bias, c2.weight, c2.bias, att[1].weight, att[1].bias, att[3].weight,
                                                   att[3].bias, self.res_scale, _pack_of(c1), _pack_of(c2)))
        if x.dtype == torch.bfloat16:   # bf16 storage (RCAN.set_act_dtype): the maps follow the dtype conv_first emitted
            return DF.rcab_bf16(x, c1.weight, c1.bias, c2.weight, c2.bias, att[1].weight, att[1].bias, att[3].weight, att[3].bias, self.res_scale,
                                _pack_of(c1), _pack_of(c2))
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
        if isinstance(x, DF.Stream32):
            return DF.Stream32(*DF.conv3x3_res_bf16_res32(t.sb, self.conv.weight, self.conv.bias, x.s, _pack_of(self.conv), out_bf16=True))
        if x.dtype == torch.bfloat16:
            return DF.conv3x3_res_bf16(t, self.conv.weight, self.conv.bias, x, _pack_of(self.conv))
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
            if x.dtype == torch.bfloat16:
                x = DF.conv3x3_ps_bf16(x, conv.weight, conv.bias, shuffle.upscale_factor, _pack_of(conv))
            else:
                x = DF.conv3x3_ps(x, conv.weight, conv.bias, shuffle.upscale_factor)
        return x


@ARCH_REGISTRY.register()
class RCAN(nn.Module):
    def __init__(self, num_in_ch, num_out_ch, num_feat=64, num_group=10, num_block=16, squeeze_factor=16, upscale=4, res_scale=1,
                 img_range=255.0, rgb_mean=(0.4488, 0.4371, 0.4040), act_dtype="fp32"):
        super().__init__()
        if act_dtype not in _ACT_DTYPES:
            raise ValueError(f"act_dtype must be one of {_ACT_DTYPES}, got {act_dtype!r}")
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
        self._num_feat = num_feat
        self.set_act_dtype(act_dtype)

    def set_act_dtype(self, act_dtype):
        """"fp32" (the reference's arithmetic), "bf16" (inference on bf16 activation storage) or "bf16_res32" (the same with the residual stream
        in fp32); the parameters are untouched"""
        if act_dtype not in _ACT_DTYPES:
            raise ValueError(f"act_dtype must be one of {_ACT_DTYPES}, got {act_dtype!r}")
        if act_dtype in _BF16_MODES and self._num_feat % 8:
            raise ValueError(f"act_dtype={act_dtype!r} needs num_feat % 8 == 0 (16-byte bf16 channel vectors), got num_feat={self._num_feat}")
        self.act_dtype = act_dtype

    def _convs_bf16(self):
        """(cache, weight) of every 3 x 3 conv of the body and the tail that has a cached bf16 operand image"""
        convs = self.__dict__.get("_bf16_convs")
        if convs is None:   # (a plain attribute, not a registered submodule list)
            convs = [m for part in (self.body, self.upsample) for m in part.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3)]
            convs.append(self.conv_after_body)
            convs = [m for m in convs if _pack_of(m) is not None]
            self.__dict__["_bf16_convs"] = convs
        return [(m._packed_bf16, m.weight) for m in convs]

    def forward(self, x):
        self.mean = self.mean.type_as(x)
        cin = x.shape[1]
        mean = self.mean.reshape(-1)
        if mean.numel() != cin:
            raise ValueError(f"RCAN: rgb_mean has {mean.numel()} entries for a {cin}-channel input")
        bf, res32 = self.act_dtype in _BF16_MODES, self.act_dtype == "bf16_res32"
        if bf:
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
                raise NotImplementedError("RCAN: bf16 storage for RCAN is inference-only (there is no bf16 backward pass); run the forward under "
                                          "torch.no_grad() or switch to set_act_dtype('fp32')")
            if x.is_cuda:   # the operand images of all 3 x 3 weights in one call where they are stale; the convs then find their pack current
                DF.pack_convs_bf16(self._convs_bf16())
        xn = DF.img_affine(x, mean, self.img_range, 0)
        x_first = DF.conv3x3_in(xn, self.conv_first.weight, self.conv_first.bias, out_bf16=bf and not res32)
        t = DF.Stream32(x_first, DF.to_bf16(x_first)) if res32 else x_first
        for group in self.body:
            t = group(t)
        if res32:   # the stream ends here: only the bf16 map the upsampler reads is written
            res = DF.conv3x3_res_bf16_res32(t.sb, self.conv_after_body.weight, self.conv_after_body.bias, x_first, _pack_of(self.conv_after_body),
                                            out_f32=False, out_bf16=True)[1]
        elif bf:
            res = DF.conv3x3_res_bf16(t, self.conv_after_body.weight, self.conv_after_body.bias, x_first, _pack_of(self.conv_after_body))
        else:
            res = DF.conv3x3_res(t, self.conv_after_body.weight, self.conv_after_body.bias, x_first)
        out = DF.conv3x3_out(self.upsample(res), self.conv_last.weight, self.conv_last.bias)
        return DF.img_affine(out, mean, self.img_range, 1)
