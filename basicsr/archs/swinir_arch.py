"""SwinIR for DCPT, MI355X-native.

Registry name ``SwinIR``, constructor kwargs, ``forward(x, hook=False)`` and ``state_dict`` keys / shapes as the reference's DCPT
variant (basicsr/archs/swinir_arch.py): window attention WITHOUT relative-position bias and WITHOUT the shift mask (odd blocks
still roll the map by -window_size // 2, so the edge windows wrap around unmasked), encoder RSTBs under ``encode_layers.{i}``
and decoder RSTBs as attributes ``decode_layers{i}``.  All four forms of the reference are built: restoration (``upsampler=''``),
classical SR (``'pixelshuffle'``, upscale 2 / 3 / 4 / 8), lightweight SR (``'pixelshuffledirect'``, 2 / 3 / 4) and real-world SR
(``'nearest+conv'``, 2 / 4), with ``resi_connection`` ``'1conv'`` or ``'3conv'`` (``embed_dim % 16 == 0``).  As in the reference, the
three SR forms add no image residual and do not undo the input normalisation.

Every Swin block is two autograd nodes: ``dcpt_swin_attn_*`` (LayerNorm in the qkv GEMM's operand loader -> window attention
kernel on the un-shifted token rows -> proj GEMM + bias + residual) and ``dcpt_swin_mlp_*`` (LayerNorm -> fc1 -> erf GELU ->
fc2 + bias + residual).  Token maps are channels_last (B, C, H, W) tensors, whose NHWC rows are the reference's (B, L, C) tokens.
Child modules only own the parameters.

``act_dtype="bf16"`` (this repo's extension, default "fp32"; ``network_g.act_dtype`` in the options, ``set_act_dtype`` on an existing network):
INFERENCE of the restoration form (``upsampler=''``, ``'1conv'``) on bf16 activation storage.  Token maps are bf16 rows PADDED to 16 bytes:
``Cp`` = embed_dim rounded up to a multiple of 8 (184 for 180, 40 for 36), heads padded to ``hdp`` = head_dim rounded up to a multiple of 8
(32 for 30), pad columns exact zeros everywhere -- they come from zero-padded operands (``pad_block_params`` and the padded conv weights,
built once per parameter version, cached per module as plain attributes and refreshed at the top of the forward where stale), not from
masking in kernels.  ``conv_first`` emits the bf16 map, every block is ``dcpt_swin_attn_fwd_bf16`` + ``dcpt_swin_mlp_fwd_bf16``, the RSTB convs
and ``conv_after_body`` are ``dcpt_conv3x3_res_fwd_bf16`` at width Cp, ``conv_last`` takes the bf16 map to the fp32 image.  Parameters,
LayerNorm statistics, scores, softmax and accumulation stay fp32; the state_dict does not depend on the mode.  There is no backward pass and
no tap pass: a bf16 forward that would have to record a graph, or ``hook=True``, raises ``NotImplementedError``.

``act_dtype="bf16_res32"``: the same inference path with the RESIDUAL STREAM -- the token map that runs through the 72 residual adds and the
RSTB convs -- kept in fp32 padded rows (``DF.Stream32``): ``conv_first`` emits fp32 at width Cp, every LayerNorm reads fp32 rows and writes
bf16, every block is ``dcpt_swin_attn_fwd_bf16_res32`` + ``dcpt_swin_mlp_fwd_bf16_res32`` (the last block of an RSTB also writes the bf16 image
its conv reads), the RSTB convs are ``dcpt_conv3x3_res_fwd_bf16_res32`` with fp32 out, ``conv_after_body`` the same with only the bf16 map
out.  Every GEMM operand is still bf16; only the stream's own rounding is gone.  Same restrictions, same parameters, same cached operands.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from basicsr.utils.registry import ARCH_REGISTRY
from dcpt_amd import functional as DF

LN_EPS = 1e-5   # nn.LayerNorm default, the reference's norm_layer
_ACT_DTYPES = ("fp32", "bf16", "bf16_res32")
_BF16_MODES = ("bf16", "bf16_res32")   # inference on bf16 maps; the second keeps the residual stream in fp32
BF16_MAX_CP = 256   # launch_conv3x3_b2s_bf16 (conv_last) and the padded-row LayerNorm hold at most 256 channels per pixel


def pad8(n: int) -> int:
    """the padding rule of the bf16 path: rows (Cp) and heads (hdp) are rounded up to a multiple of 8 elements = 16 bytes"""
    return (int(n) + 7) // 8 * 8


def _pad_to(t, shape):
    out = t.new_zeros(shape)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


def pad_block_params(blk):
    """The zero-padded fp32 parameter set of one Swin block for the bf16 path (dict; on the parameters' device, CPU included):
    norm1_w / norm1_b / norm2_w / norm2_b / proj_b / fc2_b [Cp], qkv_w [3 heads hdp][Cp] and qkv_b [3 heads hdp] with the reference's row
    s*C + h*hd + d at (s*heads + h)*hdp + d, proj_w [Cp][heads hdp] with the reference's column h*hd + d at h*hdp + d, fc1_w [hidden][Cp],
    fc1_b [hidden], fc2_w [Cp][hidden].  Pad rows, pad columns and pad entries are zero, so pad columns of every map stay exactly zero."""
    C_, heads = blk.dim, blk.num_heads
    hd = C_ // heads
    Cp, hdp = pad8(C_), pad8(hd)
    a, m = blk.attn, blk.mlp
    hidden = m.fc1.weight.shape[0]
    d = lambda t: t.detach().float()   # noqa: E731
    return {
        "norm1_w": _pad_to(d(blk.norm1.weight), (Cp,)), "norm1_b": _pad_to(d(blk.norm1.bias), (Cp,)),
        "qkv_w": _pad_to(d(a.qkv.weight).reshape(3, heads, hd, C_), (3, heads, hdp, Cp)).reshape(3 * heads * hdp, Cp),
        "qkv_b": _pad_to(d(a.qkv.bias).reshape(3, heads, hd), (3, heads, hdp)).reshape(3 * heads * hdp),
        "proj_w": _pad_to(d(a.proj.weight).reshape(C_, heads, hd), (Cp, heads, hdp)).reshape(Cp, heads * hdp),
        "proj_b": _pad_to(d(a.proj.bias), (Cp,)),
        "norm2_w": _pad_to(d(blk.norm2.weight), (Cp,)), "norm2_b": _pad_to(d(blk.norm2.bias), (Cp,)),
        "fc1_w": _pad_to(d(m.fc1.weight), (hidden, Cp)), "fc1_b": d(m.fc1.bias).clone(),
        "fc2_w": _pad_to(d(m.fc2.weight), (Cp, hidden)), "fc2_b": _pad_to(d(m.fc2.bias), (Cp,)),
    }


_BF16_IMAGES = ("qkv_w", "proj_w", "fc1_w", "fc2_w")   # the GEMM weight operands: rounded to bf16 once, here


def _cache(mod):
    if getattr(mod, "_swin_bf16", None) is None:
        mod._swin_bf16 = DF.SwinPackBf16()
    return mod._swin_bf16


def _refresh_conv(conv, cout_p, cin_p, packed=True):
    """the zero-padded weight / bias of a 3 x 3 conv at the padded width (and, for the GEMM convs, the cache of its bf16 operand images);
    returns (cache, rebuilt)"""
    pk = _cache(conv)
    if packed and pk.conv is None:
        pk.conv = DF.PackedConvBf16()

    def build():
        return {"w": _pad_to(conv.weight.detach().float(), (cout_p, cin_p, 3, 3)), "b": _pad_to(conv.bias.detach().float(), (cout_p,))}

    return pk, pk.refresh((conv.weight, conv.bias), build)


def _refresh_norm(norm, Cp):
    pk = _cache(norm)
    return pk, pk.refresh((norm.weight, norm.bias), lambda: {"w": _pad_to(norm.weight.detach().float(), (Cp,)),
                                                             "b": _pad_to(norm.bias.detach().float(), (Cp,))})


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

    def _params(self):
        a, m = self.attn, self.mlp
        return (self.norm1.weight, self.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, self.norm2.weight, self.norm2.bias,
                m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)

    def refresh_bf16(self) -> bool:
        """the block's padded operands for the bf16 path, rebuilt if a parameter changed; True if they were"""

        def build():
            P = pad_block_params(self)
            return {k: (v.to(torch.bfloat16) if k in _BF16_IMAGES else v).contiguous() for k, v in P.items()}

        return _cache(self).refresh(self._params(), build)

    def _forward_bf16(self, x):
        self.refresh_bf16()
        t = self._swin_bf16.t
        x = DF.swin_attn_bf16(x, (t["norm1_w"], t["norm1_b"], t["qkv_w"], t["qkv_b"], t["proj_w"], t["proj_b"]), self.dim, self.num_heads,
                              pad8(self.dim // self.num_heads), self.window_size, self.shift_size)
        return DF.swin_mlp_bf16(x, (t["norm2_w"], t["norm2_b"], t["fc1_w"], t["fc1_b"], t["fc2_w"], t["fc2_b"]), self.dim)

    def _forward_res32(self, x, out_bf16, inplace=False):
        """the block on the fp32 residual stream x (padded rows); ``out_bf16``: the MLP half also writes the stream's bf16 image; ``inplace``: the
        stream is updated where it lies (x is the caller's own map: an RSTB's blocks after its first) -- the MLP half always updates the
        attention half's output in place, so a block holds one fp32 map, or none, besides its input"""
        self.refresh_bf16()
        t = self._swin_bf16.t
        x = DF.swin_attn_bf16_res32(x, (t["norm1_w"], t["norm1_b"], t["qkv_w"], t["qkv_b"], t["proj_w"], t["proj_b"]), self.dim, self.num_heads,
                                    pad8(self.dim // self.num_heads), self.window_size, self.shift_size, inplace=inplace)
        return DF.Stream32(*DF.swin_mlp_bf16_res32(x, (t["norm2_w"], t["norm2_b"], t["fc1_w"], t["fc1_b"], t["fc2_w"], t["fc2_b"]), self.dim,
                                                   out_bf16=out_bf16, inplace=True))

    def forward(self, x):
        if isinstance(x, DF.Stream32):   # bf16 maps around the fp32 residual stream
            return self._forward_res32(x.s, True)
        if x.dtype == torch.bfloat16:   # bf16 storage (SwinIR.set_act_dtype): the maps follow the dtype conv_first emitted
            return self._forward_bf16(x)
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


def _residual_conv(dim, resi_connection):
    """the reference's ``conv`` / ``conv_after_body``: one 3x3 conv, or the 3conv bottleneck whose LeakyReLUs (indices 1, 3) own nothing"""
    if resi_connection == "1conv":
        return nn.Conv2d(dim, dim, 3, 1, 1)
    return nn.Sequential(nn.Conv2d(dim, dim // 4, 3, 1, 1), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                         nn.Conv2d(dim // 4, dim // 4, 1, 1, 0), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                         nn.Conv2d(dim // 4, dim, 3, 1, 1))


def _apply_residual_conv(conv, t, res):
    """res + conv(t) as one autograd node"""
    if isinstance(conv, nn.Conv2d):
        return DF.conv3x3_res(t, conv.weight, conv.bias, res)
    return DF.conv3conv_res(t, conv[0].weight, conv[0].bias, conv[2].weight, conv[2].bias, conv[4].weight, conv[4].bias, res)


def _conv_res_bf16(conv, t, res):
    """bf16(res + conv(t)) at the padded width, from the conv's padded weight and its cached operand image"""
    Cp = t.shape[1]
    pk, _ = _refresh_conv(conv, Cp, Cp)
    return DF.conv3x3_res_bf16(t, pk.t["w"], pk.t["b"], res, pk.conv)


def _conv_res_res32(conv, t, res, stream_out):
    """res + conv(t) at the padded width from the fp32 accumulator, t bf16 and res fp32: the new fp32 stream (``stream_out``), or only its bf16
    map where the stream ends"""
    Cp = t.shape[1]
    pk, _ = _refresh_conv(conv, Cp, Cp)
    y, yb = DF.conv3x3_res_bf16_res32(t, pk.t["w"], pk.t["b"], res, pk.conv, out_f32=stream_out, out_bf16=not stream_out)
    return DF.Stream32(y, None) if stream_out else yb


class RSTB(nn.Module):
    """residual Swin group: x + conv(blocks(x)), conv = one 3x3 conv or the 3conv bottleneck."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio, resi_connection="1conv"):
        super().__init__()
        self.residual_group = BasicLayer(dim, input_resolution, depth, num_heads, window_size, mlp_ratio)
        self.conv = _residual_conv(dim, resi_connection)

    def forward(self, x):
        if isinstance(x, DF.Stream32):   # only the last block writes the bf16 image of the stream: the conv's operand
            blocks, t = self.residual_group.blocks, x
            for i, blk in enumerate(blocks):   # the first block leaves x (the conv's residual) alone, the others update their own map in place
                t = blk._forward_res32(t.s, i == len(blocks) - 1, inplace=i > 0)
            sb = t.sb
            del t   # (the stream's fp32 map is dead once its bf16 image exists: not held while the conv's output is allocated)
            return _conv_res_res32(self.conv, sb, x.s, True)
        t = x
        for blk in self.residual_group.blocks:
            t = blk(t)
        if x.dtype == torch.bfloat16:
            return _conv_res_bf16(self.conv, t, x)
        return _apply_residual_conv(self.conv, t, x)


class Upsample(nn.Sequential):
    """classical upsampler: (conv3x3 C -> 4C, PixelShuffle(2)) per factor of two, or one (conv3x3 C -> 9C, PixelShuffle(3)); the convs sit at
    the even indices, as in the reference; each stage runs as one DF.conv3x3_ps node"""

    def __init__(self, scale, num_feat):
        m = []
        if scale & (scale - 1) == 0:
            for _ in range(scale.bit_length() - 1):
                m += [nn.Conv2d(num_feat, 4 * num_feat, 3, 1, 1), nn.PixelShuffle(2)]
        elif scale == 3:
            m += [nn.Conv2d(num_feat, 9 * num_feat, 3, 1, 1), nn.PixelShuffle(3)]
        else:
            raise ValueError(f"scale {scale} is not supported. Supported scales: 2^n and 3.")
        super().__init__(*m)

    def forward(self, x):
        for i in range(0, len(self), 2):
            x = DF.conv3x3_ps(x, self[i].weight, self[i].bias, self[i + 1].upscale_factor)
        return x


class UpsampleOneStep(nn.Sequential):
    """lightweight upsampler: conv3x3 C -> r^2 num_out_ch + PixelShuffle(r), written as the NCHW image by one DF.conv3x3_ps_out node"""

    def __init__(self, scale, num_feat, num_out_ch):
        super().__init__(nn.Conv2d(num_feat, scale * scale * num_out_ch, 3, 1, 1), nn.PixelShuffle(scale))

    def forward(self, x):
        return DF.conv3x3_ps_out(x, self[0].weight, self[0].bias, self[1].upscale_factor)


SR_SCALES = {"pixelshuffle": (2, 3, 4, 8), "pixelshuffledirect": (2, 3, 4), "nearest+conv": (2, 4)}
NUM_FEAT = 64   # the reference's fixed width of the reconstruction tail


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
                 resi_connection="1conv", act_dtype="fp32", **kwargs):
        super().__init__()
        if act_dtype not in _ACT_DTYPES:
            raise ValueError(f"act_dtype must be one of {_ACT_DTYPES}, got {act_dtype!r}")
        if upsampler == "":
            if upscale != 1:
                raise NotImplementedError(f"upscale={upscale} without an upsampler: the restoration form (upsampler '') has upscale 1")
        elif upsampler not in SR_SCALES:
            raise NotImplementedError(f"upsampler={upsampler!r}: one of '', 'pixelshuffle', 'pixelshuffledirect', 'nearest+conv'")
        elif upscale not in SR_SCALES[upsampler]:
            raise NotImplementedError(f"upsampler={upsampler!r} with upscale={upscale}: the DCPT path has upscale in {SR_SCALES[upsampler]}"
                                      + (" (the reference silently builds x2 for any other value)" if upsampler == "nearest+conv" else ""))
        if upsampler == "pixelshuffledirect" and in_chans > 4:
            raise NotImplementedError(f"upsampler='pixelshuffledirect' with in_chans={in_chans}: at most 4 image channels")
        if resi_connection not in ("1conv", "3conv"):
            raise NotImplementedError(f"resi_connection={resi_connection!r}: '1conv' or '3conv'")
        if resi_connection == "3conv" and embed_dim % 16:
            raise NotImplementedError(f"resi_connection='3conv' with embed_dim={embed_dim}: the inner maps are embed_dim // 4 = {embed_dim // 4} "
                                      "channels wide and the NHWC kernels work on float4 channel groups, so embed_dim must be a multiple "
                                      "of 16 (the default width 180 is not; the published 3conv model is 240 wide)")
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
            RSTB(embed_dim, res, depths[i], num_heads[i], window_size, mlp_ratio, resi_connection) for i in range(half))
        for i in range(half):
            setattr(self, f"decode_layers{i}", RSTB(embed_dim, res, depths[i + 3], num_heads[i + 3], window_size, mlp_ratio, resi_connection))
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = _residual_conv(embed_dim, resi_connection)
        # reconstruction (reference :981-1011; num_feat = 64 and num_out_ch = in_chans are fixed there)
        if upsampler == "pixelshuffle":
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, NUM_FEAT, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.upsample = Upsample(upscale, NUM_FEAT)
            self.conv_last = nn.Conv2d(NUM_FEAT, in_chans, 3, 1, 1)
        elif upsampler == "pixelshuffledirect":
            self.upsample = UpsampleOneStep(upscale, embed_dim, in_chans)
        elif upsampler == "nearest+conv":
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, NUM_FEAT, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.conv_up1 = nn.Conv2d(NUM_FEAT, NUM_FEAT, 3, 1, 1)
            if upscale == 4:
                self.conv_up2 = nn.Conv2d(NUM_FEAT, NUM_FEAT, 3, 1, 1)
            self.conv_hr = nn.Conv2d(NUM_FEAT, NUM_FEAT, 3, 1, 1)
            self.conv_last = nn.Conv2d(NUM_FEAT, in_chans, 3, 1, 1)
            self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        else:
            self.conv_last = nn.Conv2d(embed_dim, in_chans, 3, 1, 1)
        self.resi_connection = resi_connection
        self.apply(self._init_weights)
        self.pack_builds = 0   # how many cached operand sets the bf16 forwards have (re)built so far
        self.set_act_dtype(act_dtype)

    def set_act_dtype(self, act_dtype):
        """"fp32" (the reference's arithmetic), "bf16" (inference of the restoration form on bf16 activation storage) or "bf16_res32" (the same
        with the residual stream in fp32); parameters untouched"""
        if act_dtype not in _ACT_DTYPES:
            raise ValueError(f"act_dtype must be one of {_ACT_DTYPES}, got {act_dtype!r}")
        if act_dtype in _BF16_MODES:
            if self.upsampler != "":
                raise NotImplementedError(f"act_dtype={act_dtype!r} with upsampler={self.upsampler!r}: bf16 storage covers the restoration form (upsampler '') only")
            if self.resi_connection == "3conv":
                raise NotImplementedError(f"act_dtype={act_dtype!r} with resi_connection='3conv': bf16 storage covers '1conv' only")
            if pad8(self.embed_dim) > BF16_MAX_CP:
                raise NotImplementedError(f"act_dtype={act_dtype!r} with embed_dim={self.embed_dim}: the padded width {pad8(self.embed_dim)} is above "
                                          f"{BF16_MAX_CP} (the ending conv and the padded-row LayerNorm hold at most {BF16_MAX_CP} channels per pixel)")
            for layer in self.layers():
                for blk in layer.residual_group.blocks:
                    hidden = blk.mlp.fc1.weight.shape[0]
                    if hidden % 8:
                        raise NotImplementedError(f"act_dtype={act_dtype!r} with an mlp hidden width of {hidden}: it must be a multiple of 8")
        self.act_dtype = act_dtype

    def padded_dim(self) -> int:
        """Cp: the row length of the bf16 token maps (embed_dim rounded up to a multiple of 8)"""
        return pad8(self.embed_dim)

    def _refresh_bf16(self):
        """every stale padded operand set of the network rebuilt, the 3 x 3 operand images of the GEMM convs in one pack call"""
        Cp, n = self.padded_dim(), 0
        n += _refresh_conv(self.conv_first, Cp, self.conv_first.in_channels, packed=False)[1]
        n += _refresh_conv(self.conv_last, self.conv_last.out_channels, Cp, packed=False)[1]
        for norm in (self.patch_embed.norm, self.norm):
            if norm is not None:
                n += _refresh_norm(norm, Cp)[1]
        convs = []
        for layer in self.layers():
            n += sum(blk.refresh_bf16() for blk in layer.residual_group.blocks)
            convs.append(layer.conv)
        convs.append(self.conv_after_body)
        for conv in convs:
            n += _refresh_conv(conv, Cp, Cp)[1]
        DF.pack_convs_bf16([(c._swin_bf16.conv, c._swin_bf16.t["w"]) for c in convs])
        self.pack_builds += n
        return n

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

    def _forward_bf16(self, xn, mean):
        """the restoration form on bf16 rows of padded_dim() channels: no torch op touches a feature map"""
        self._refresh_bf16()
        C_ = self.embed_dim
        res32 = self.act_dtype == "bf16_res32"
        ln = DF.ln_pad_bf16_res32 if res32 else DF.ln_pad_bf16
        first, last = self.conv_first._swin_bf16.t, self.conv_last._swin_bf16.t
        x_first = DF.conv3x3_in(xn, first["w"], first["b"], out_bf16=not res32)
        t = x_first
        if self.patch_embed.norm is not None:
            pn = self.patch_embed.norm._swin_bf16.t
            t = ln(t, pn["w"], pn["b"], C_, LN_EPS)
            if res32:   # a LayerNorm output is a bf16 storage point; the stream starts from that value, exactly
                t = DF.to_f32(t)
        if res32:
            t = DF.Stream32(t, None)
        for layer in self.layers():
            t = layer(t)
        fn = self.norm._swin_bf16.t
        t = ln(t.s if res32 else t, fn["w"], fn["b"], C_, LN_EPS)
        if res32:   # the stream ends here: only the bf16 map conv_last reads is written
            res = _conv_res_res32(self.conv_after_body, t, x_first, False)
        else:
            res = _conv_res_bf16(self.conv_after_body, t, x_first)
        out = DF.conv3x3_out(res, last["w"], last["b"], xn)
        return DF.img_affine(out, mean, self.img_range, 1)

    def forward(self, x, hook=False):
        bf = self.act_dtype in _BF16_MODES
        if bf:   # (before anything else, CPU tensors included)
            if hook:
                raise NotImplementedError("SwinIR: bf16 storage for SwinIR is inference-only: the tap pass (hook=True) belongs to training; "
                                          "switch to set_act_dtype('fp32')")
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
                raise NotImplementedError("SwinIR: bf16 storage for SwinIR is inference-only (there is no bf16 backward pass); run the forward under "
                                          "torch.no_grad() or switch to set_act_dtype('fp32')")
        _, cin, H, W = x.shape
        ws = self.block_window()
        if H % ws or W % ws:
            raise ValueError(f"SwinIR: input {H} x {W} is not a multiple of the window size {ws} (pad it first, as SRModel.pre_test does)")
        self.mean = self.mean.type_as(x)
        mean = self.mean.reshape(-1).expand(cin) if self.mean.numel() == 1 else self.mean.reshape(-1)
        xn = DF.img_affine(x, mean, self.img_range, 0)
        if bf:
            return self._forward_bf16(xn, mean)
        x_first = DF.conv3x3_in(xn, self.conv_first.weight, self.conv_first.bias)
        t = x_first
        if self.patch_embed.norm is not None:
            t = DF.layernorm2d(t, self.patch_embed.norm.weight, self.patch_embed.norm.bias, LN_EPS)
        for layer in self.layers():
            t = layer(t)
        if hook:   # the tap pass of the DCPT step: the forward hooks on decode_layers{i} have fired and the caller drops the image (the
            return None   # reference computes the tail and discards it, ...pretrain_model.py:154; NAFNetBaseline returns None here too)
        t = DF.layernorm2d(t, self.norm.weight, self.norm.bias, LN_EPS)
        res = _apply_residual_conv(self.conv_after_body, t, x_first)
        if self.upsampler == "":
            out = DF.conv3x3_out(res, self.conv_last.weight, self.conv_last.bias, xn)
            return DF.img_affine(out, mean, self.img_range, 1)
        # the SR branches (reference :1069-1100) add no image residual and leave the output in the normalised range
        if self.upsampler == "pixelshuffledirect":
            return self.upsample(res)
        cb = self.conv_before_upsample[0]
        t = DF.conv3x3_act(res, cb.weight, cb.bias, self.conv_before_upsample[1].negative_slope)
        if self.upsampler == "pixelshuffle":
            t = self.upsample(t)
        else:
            slope = self.lrelu.negative_slope
            t = DF.up2_conv3x3_act(t, self.conv_up1.weight, self.conv_up1.bias, slope)
            if self.upscale == 4:
                t = DF.up2_conv3x3_act(t, self.conv_up2.weight, self.conv_up2.bias, slope)
            t = DF.conv3x3_act(t, self.conv_hr.weight, self.conv_hr.bias, slope)
        return DF.conv3x3_out(t, self.conv_last.weight, self.conv_last.bias)
