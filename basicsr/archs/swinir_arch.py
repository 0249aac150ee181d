"""SwinIR for DCPT, MI355X-native.

Registry name ``SwinIR``, constructor kwargs, ``forward(x, hook=False)`` and ``state_dict`` keys / shapes as the reference's DCPT
variant (basicsr/archs/swinir_arch.py): window attention WITHOUT relative-position bias and WITHOUT the shift mask (odd blocks
still roll the map by -window_size // 2, so the edge windows wrap around unmasked), encoder RSTBs under ``encode_layers.{i}``
and decoder RSTBs as attributes ``decode_layers{i}``, ``upsampler=''`` / ``upscale=1`` only.

Every Swin block is two autograd nodes: ``dcpt_swin_attn_*`` (LayerNorm in the qkv GEMM's operand loader -> window attention
kernel on the un-shifted token rows -> proj GEMM + bias + residual) and ``dcpt_swin_mlp_*`` (LayerNorm -> fc1 -> erf GELU ->
fc2 + bias + residual).  Token maps are channels_last (B, C, H, W) tensors, whose NHWC rows are the reference's (B, L, C) tokens.
Child modules only own the parameters.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from basicsr.utils.registry import ARCH_REGISTRY
from dcpt_amd import functional as DF

LN_EPS = 1e-5   # nn.LayerNorm default, the reference's norm_layer


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class WindowAttention(nn.Module):
    def __init__(self, dim, window_size, num_heads):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.proj = nn.Linear(dim, dim)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, input_resolution, num_heads, window_size, shift_size, mlp_ratio):
        super().__init__()
        self.dim, self.num_heads, self.mlp_ratio = dim, num_heads, mlp_ratio
        self.input_resolution = input_resolution
        # the window is fixed by the CONSTRUCTOR's resolution (img_size), not by the image seen at run time
        if min(input_resolution) <= window_size:
            window_size, shift_size = min(input_resolution), 0
        self.window_size, self.shift_size = window_size, shift_size
        if window_size * window_size > 64:
            raise NotImplementedError(f"window_size {window_size}: the window kernel holds at most 64 tokens per window")
        if dim % 4 or dim % num_heads or dim // num_heads > 64:
            raise NotImplementedError(f"dim={dim}, num_heads={num_heads}: needs dim % 4 == 0, dim % heads == 0, head_dim <= 64")
        hidden = int(dim * mlp_ratio)
        if hidden % 4:
            raise NotImplementedError(f"mlp hidden width {hidden} must be a multiple of 4")
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, (window_size, window_size), num_heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, hidden)

    def forward(self, x):
        a, m = self.attn, self.mlp
        x = DF.swin_attn(x, self.norm1.weight, self.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, self.num_heads,
                         self.window_size, self.shift_size)
        return DF.swin_mlp(x, self.norm2.weight, self.norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)


class BasicLayer(nn.Module):
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio):
        super().__init__()
        self.blocks = nn.ModuleList(
            SwinTransformerBlock(dim, input_resolution, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2, mlp_ratio)
            for i in range(depth))


class RSTB(nn.Module):
    """residual Swin group: x + conv3x3(blocks(x)) + bias."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio):
        super().__init__()
        self.residual_group = BasicLayer(dim, input_resolution, depth, num_heads, window_size, mlp_ratio)
        self.conv = nn.Conv2d(dim, dim, 3, 1, 1)

    def forward(self, x):
        t = x
        for blk in self.residual_group.blocks:
            t = blk(t)
        return DF.conv3x3_res(t, self.conv.weight, self.conv.bias, x)


class PatchEmbed(nn.Module):
    """holds the LayerNorm that follows conv_first (patch_norm=True); the flatten itself is the NHWC layout."""

    def __init__(self, embed_dim, patch_norm):
        super().__init__()
        self.norm = nn.LayerNorm(embed_dim) if patch_norm else None


@ARCH_REGISTRY.register()
class SwinIR(nn.Module):
    def __init__(self, img_size=128, patch_size=1, in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=(6, 6, 6, 6, 6, 6),
                 window_size=8, mlp_ratio=2.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 norm_layer=nn.LayerNorm, ape=False, patch_norm=True, use_checkpoint=False, upscale=1, img_range=1.0, upsampler="",
                 resi_connection="1conv", **kwargs):
        super().__init__()
        if upsampler != "" or upscale != 1:
            raise NotImplementedError(f"upsampler={upsampler!r} / upscale={upscale}: only the restoration form (upsampler '', upscale 1) "
                                      "is on the DCPT path")
        if resi_connection != "1conv":
            raise NotImplementedError(f"resi_connection={resi_connection!r}: only '1conv' is on the DCPT path")
        if ape:
            raise NotImplementedError("ape=True (absolute position embedding) is not on the DCPT path")
        if drop_rate > 0 or attn_drop_rate > 0 or drop_path_rate > 0:
            raise NotImplementedError("dropout / drop path are not on the DCPT path (drop_rate, attn_drop_rate, drop_path_rate must be 0)")
        if not qkv_bias or qk_scale is not None:
            raise NotImplementedError("qkv_bias=False / qk_scale are not on the DCPT path")
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("norm_layer must be nn.LayerNorm")
        depths, num_heads = list(depths), list(num_heads)
        if len(depths) % 2 or len(num_heads) != len(depths):
            raise ValueError("depths / num_heads: an even number of layers, one head count per layer")
        self.img_range = img_range
        self.mean = torch.Tensor((0.4488, 0.4371, 0.4040)).view(1, 3, 1, 1) if in_chans == 3 else torch.zeros(1, 1, 1, 1)
        self.upscale, self.upsampler, self.window_size = upscale, upsampler, window_size
        self.num_layers, self.embed_dim, self.num_features = len(depths), embed_dim, embed_dim
        self.ape, self.patch_norm, self.mlp_ratio = ape, patch_norm, mlp_ratio
        self.use_checkpoint = use_checkpoint   # accepted; recomputation would give the same results
        img = _pair(img_size)
        ps = _pair(patch_size)
        res = (img[0] // ps[0], img[1] // ps[1])
        self.patches_resolution = list(res)

        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = PatchEmbed(embed_dim, patch_norm)
        half = self.num_layers // 2
        self.encode_layers = nn.ModuleList(
            RSTB(embed_dim, res, depths[i], num_heads[i], window_size, mlp_ratio) for i in range(half))
        for i in range(half):
            setattr(self, f"decode_layers{i}", RSTB(embed_dim, res, depths[i + 3], num_heads[i + 3], window_size, mlp_ratio))
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1)
        self.conv_last = nn.Conv2d(embed_dim, in_chans, 3, 1, 1)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def layers(self):
        return list(self.encode_layers) + [getattr(self, f"decode_layers{i}") for i in range(self.num_layers // 2)]

    def block_window(self) -> int:
        return self.encode_layers[0].residual_group.blocks[0].window_size

    def forward(self, x, hook=False):
        _, cin, H, W = x.shape
        ws = self.block_window()
        if H % ws or W % ws:
            raise ValueError(f"SwinIR: input {H} x {W} is not a multiple of the window size {ws} (pad it first, as SRModel.pre_test does)")
        self.mean = self.mean.type_as(x)
        mean = self.mean.reshape(-1).expand(cin) if self.mean.numel() == 1 else self.mean.reshape(-1)
        xn = DF.img_affine(x, mean, self.img_range, 0)
        x_first = DF.conv3x3_in(xn, self.conv_first.weight, self.conv_first.bias)
        t = x_first
        if self.patch_embed.norm is not None:
            t = DF.layernorm2d(t, self.patch_embed.norm.weight, self.patch_embed.norm.bias, LN_EPS)
        for layer in self.layers():
            t = layer(t)
        t = DF.layernorm2d(t, self.norm.weight, self.norm.bias, LN_EPS)
        res = DF.conv3x3_res(t, self.conv_after_body.weight, self.conv_after_body.bias, x_first)
        out = DF.conv3x3_out(res, self.conv_last.weight, self.conv_last.bias, xn)
        return DF.img_affine(out, mean, self.img_range, 1)
