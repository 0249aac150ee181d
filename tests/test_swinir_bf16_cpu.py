"""SwinIR on bf16 activation storage, the parts that need no GPU: constructor / set_act_dtype validation, state_dict keys, the inference-only
checks, the device-free workspace queries, the argument checks of dcpt_swin_attn_fwd_bf16 / dcpt_swin_mlp_fwd_bf16 / dcpt_ln_pad_fwd_bf16
(refused before any launch) and the PADDING MAP: the product's own pack function (swinir_arch.pad_block_params) against a plain-torch Swin
block run over zero-padded rows."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

TINY = dict(embed_dim=36, depths=[2] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)


@pytest.fixture(scope="module")
def lib():
    from dcpt_amd import _lib

    return _lib.load()


def _build(**kw):
    from basicsr.archs import build_network

    return build_network(dict(type="SwinIR", **dict(TINY, **kw)))


# ---- public surface ----------------------------------------------------------------------------------------------------------------------
def test_unknown_act_dtype_is_a_value_error():
    with pytest.raises(ValueError, match="act_dtype"):
        _build(act_dtype="fp16")
    net = _build()
    assert net.act_dtype == "fp32"
    with pytest.raises(ValueError, match="act_dtype"):
        net.set_act_dtype("half")
    assert net.act_dtype == "fp32"


@pytest.mark.parametrize("kw", [dict(upsampler="pixelshuffle", upscale=2), dict(upsampler="pixelshuffledirect", upscale=3),
                                dict(upsampler="nearest+conv", upscale=4)])
def test_sr_forms_are_refused(kw):
    with pytest.raises(NotImplementedError, match="upsampler"):
        _build(act_dtype="bf16", **kw)
    net = _build(**kw)
    with pytest.raises(NotImplementedError, match="upsampler"):
        net.set_act_dtype("bf16")
    assert net.act_dtype == "fp32"


def test_3conv_is_refused():
    with pytest.raises(NotImplementedError, match="3conv"):
        _build(act_dtype="bf16", embed_dim=48, resi_connection="3conv")
    net = _build(embed_dim=48, resi_connection="3conv")
    with pytest.raises(NotImplementedError, match="3conv"):
        net.set_act_dtype("bf16")


def test_padded_width_above_256_is_refused():
    with pytest.raises(NotImplementedError, match="256"):
        _build(act_dtype="bf16", embed_dim=264)   # (6 heads of 44)
    net = _build(embed_dim=252)                   # 252 -> 256: the widest that is taken
    net.set_act_dtype("bf16")
    assert net.padded_dim() == 256


def test_hidden_width_must_be_a_multiple_of_8():
    net = _build(mlp_ratio=1.0)   # hidden 36: fine for fp32 (% 4)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        net.set_act_dtype("bf16")


def test_options_spelling_and_padded_sizes():
    from basicsr.archs.swinir_arch import pad8

    net = _build(act_dtype="bf16")
    assert net.act_dtype == "bf16" and net.padded_dim() == pad8(36) == 40
    assert [pad8(n) for n in (180, 36, 30, 6, 64, 28)] == [184, 40, 32, 8, 64, 32]
    assert _build(embed_dim=180, act_dtype="bf16").padded_dim() == 184


def test_state_dict_does_not_depend_on_act_dtype():
    a, b = _build(), _build(act_dtype="bf16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys()) and len(sb) == 166
    assert all(sa[k].shape == sb[k].shape and sb[k].dtype == torch.float32 for k in sa)
    b.set_act_dtype("fp32")
    b.set_act_dtype("bf16")
    assert list(b.state_dict().keys()) == list(sa.keys())
    # the operand caches are plain attributes: building one changes nothing
    blk = b.encode_layers[0].residual_group.blocks[0]
    assert blk.refresh_bf16() is True and blk.refresh_bf16() is False
    assert blk._swin_bf16.t["qkv_w"].dtype == torch.bfloat16 and blk._swin_bf16.t["qkv_b"].dtype == torch.float32
    assert list(b.state_dict().keys()) == list(sa.keys())
    assert all(p.dtype == torch.float32 for p in b.parameters())
    with torch.no_grad():
        blk.attn.qkv.weight.mul_(2.0)
    assert blk.refresh_bf16() is True   # keyed on the parameters' _version
    b.load_state_dict(sa)
    assert blk.refresh_bf16() is True and blk.refresh_bf16() is False


def test_inference_only_is_checked_before_anything_runs():
    net = _build(act_dtype="bf16")
    with pytest.raises(NotImplementedError, match="inference-only"):
        net(torch.zeros(1, 3, 8, 8))                                   # parameters require grad, grad mode on
    net.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="inference-only"):
        net(torch.zeros(1, 3, 8, 8, requires_grad=True))               # the input requires grad
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="inference-only"):
            net(torch.zeros(1, 3, 8, 8), hook=True)                    # the tap pass belongs to training


def test_cpu_tensors_raise(lib):
    from dcpt_amd import functional as DF
    from dcpt_amd._lib import DcptHipError

    net = _build(act_dtype="bf16")
    x = torch.zeros(1, 40, 8, 8, dtype=torch.bfloat16)
    with torch.no_grad():
        with pytest.raises(DcptHipError):
            net(torch.zeros(1, 3, 8, 8))
        with pytest.raises(DcptHipError):
            DF.ln_pad_bf16(x, torch.zeros(40), torch.zeros(40), 36)
        with pytest.raises(DcptHipError):
            net.encode_layers[0].residual_group.blocks[0](x)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
NEW_NAMES = ("dcpt_ln_pad_fwd_bf16", "dcpt_swin_attn_bf16_ws_bytes", "dcpt_swin_attn_fwd_bf16", "dcpt_swin_mlp_bf16_ws_bytes",
             "dcpt_swin_mlp_fwd_bf16")


def test_abi_version_unchanged(lib):
    from dcpt_amd import _lib

    assert lib.dcpt_abi_version() == _lib.ABI_VERSION == 16
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_ws_queries_need_no_device(lib):
    att, mlp = lib.dcpt_swin_attn_bf16_ws_bytes, lib.dcpt_swin_mlp_bf16_ws_bytes
    # (B, H, W, C, Cp, heads, hdp, window) / (B, H, W, C, Cp, hidden)
    assert att(2, 16, 24, 180, 184, 6, 32, 8) > 0 and att(3, 8, 8, 36, 40, 6, 8, 8) > 0 and att(1, 14, 21, 56, 56, 2, 32, 7) > 0
    assert att(2, 12, 8, 64, 64, 1, 64, 4) > 0
    assert mlp(2, 16, 24, 180, 184, 360) > 0 and mlp(3, 8, 8, 36, 40, 72) > 0
    assert att(2, 16, 24, 180, 180, 6, 32, 8) == 0    # Cp % 8
    assert att(2, 16, 24, 180, 176, 6, 32, 8) == 0    # C > Cp
    assert att(2, 16, 24, 180, 184, 6, 24, 8) == 0    # hdp < hd
    assert att(2, 16, 24, 180, 184, 6, 30, 8) == 0    # hdp % 8
    assert att(2, 18, 27, 180, 184, 6, 32, 9) == 0    # ws^2 > 64
    assert att(2, 16, 20, 180, 184, 6, 32, 8) == 0    # W % ws
    assert att(2, 12, 24, 180, 184, 6, 32, 8) == 0    # H % ws
    assert att(0, 16, 24, 180, 184, 6, 32, 8) == 0    # B = 0
    assert att(2, 16, 24, 180, 184, 7, 32, 8) == 0    # C % heads
    assert att(2, 16, 24, 180, 264, 6, 32, 8) == 0    # Cp > 256
    assert mlp(2, 16, 24, 180, 180, 360) == 0         # Cp % 8
    assert mlp(2, 16, 24, 180, 176, 360) == 0         # C > Cp
    assert mlp(0, 16, 24, 180, 184, 360) == 0         # B = 0
    assert mlp(2, 16, 24, 180, 184, 364) == 0         # hidden % 8


def test_bad_arguments_return_an_error_instead_of_crashing(lib):
    from dcpt_amd._lib import SwinAttnBf16Params, SwinMlpBf16Params

    # host memory stands in for device buffers: every call below must be refused before it touches them
    buf = (C.c_char * (1 << 16))()
    p = C.addressof(buf)
    geo = (1, 8, 8, 36, 40, 6, 8, 8)
    pa, pm = SwinAttnBf16Params(p, p, p, p, p, p), SwinMlpBf16Params(p, p, p, p, p, p)
    need = lib.dcpt_swin_attn_bf16_ws_bytes(*geo)
    assert need > 0

    def refused(rc, what):
        assert rc != 0
        msg = lib.dcpt_last_error().decode()
        assert what in msg, msg

    att = lib.dcpt_swin_attn_fwd_bf16
    refused(att(None, p, p, p, need, *geo, 0, None), "null")
    refused(att(C.byref(pa), None, p, p, need, *geo, 0, None), "null")
    refused(att(C.byref(SwinAttnBf16Params(p, p, None, p, p, p)), p, p, p, need, *geo, 0, None), "null")
    refused(att(C.byref(pa), p, p, p, need, 1, 8, 8, 36, 36, 6, 8, 8, 0, None), "Cp a multiple of 8")
    refused(att(C.byref(pa), p, p, p, need, 1, 8, 8, 36, 40, 6, 4, 8, 0, None), "hdp")
    refused(att(C.byref(pa), p, p, p, need, 1, 9, 9, 36, 40, 6, 8, 9, 0, None), "window")
    refused(att(C.byref(pa), p, p, p, need, *geo, 8, None), "shift")
    refused(att(C.byref(pa), p, p, p, need, *geo, -1, None), "shift")
    refused(att(C.byref(pa), p, p, p, need - 1, *geo, 0, None), "workspace too small")
    refused(att(C.byref(pa), p, p, None, need, *geo, 0, None), "workspace too small")

    mgeo = (1, 8, 8, 36, 40, 72)
    need = lib.dcpt_swin_mlp_bf16_ws_bytes(*mgeo)
    mlp = lib.dcpt_swin_mlp_fwd_bf16
    refused(mlp(None, p, p, p, need, *mgeo, None), "null")
    refused(mlp(C.byref(pm), p, None, p, need, *mgeo, None), "null")
    refused(mlp(C.byref(SwinMlpBf16Params(p, p, p, p, p, None)), p, p, p, need, *mgeo, None), "null")
    refused(mlp(C.byref(pm), p, p, p, need, 1, 8, 8, 36, 40, 36, None), "hidden")
    refused(mlp(C.byref(pm), p, p, p, need, 1, 8, 8, 44, 40, 72, None), "C <= Cp")
    refused(mlp(C.byref(pm), p, p, p, need - 1, *mgeo, None), "workspace too small")
    refused(mlp(C.byref(pm), p, p, None, need, *mgeo, None), "workspace too small")

    ln = lib.dcpt_ln_pad_fwd_bf16
    refused(ln(None, p, p, p, 64, 36, 40, 1e-5, None), "null")
    refused(ln(p, p, p, p, 64, 36, 36, 1e-5, None), "multiple of 8")
    refused(ln(p, p, p, p, 64, 44, 40, 1e-5, None), "C <= Cp")
    refused(ln(p, p, p, p, 0, 36, 40, 1e-5, None), "M=0")
    assert bytes(buf) == bytes(len(buf)), "a refused call wrote into its buffers"


# ---- the padding map ----------------------------------------------------------------------------------------------------------------------
def _block(C_, heads, ws, shift, seed):
    from basicsr.archs.swinir_arch import SwinTransformerBlock
    from dcpt_amd.keyed_init import keyed_tensor

    blk = SwinTransformerBlock(C_, (128, 128), heads, ws, shift, 2.0)
    # (keyed values for every parameter: LayerNorm affine and biases away from their 1 / 0 initial values)
    blk.load_state_dict({k: keyed_tensor(f"swpad{seed}." + k, tuple(v.shape)) for k, v in blk.state_dict().items()}, strict=True)
    return blk


def _ln_real(t, w, b, C_):
    """LayerNorm over the first C_ channels of padded rows; w / b zero-padded, so pad columns come out as 0 * 0 + 0"""
    real = t[..., :C_]
    mu = real.mean(-1, keepdim=True)
    var = ((real - mu) ** 2).mean(-1, keepdim=True)
    mask = torch.zeros(t.shape[-1])
    mask[:C_] = 1.0
    return ((t - mu) * mask) / torch.sqrt(var + 1e-5) * w + b


def padded_block(xp, P, C_, heads, hdp, ws, shift):
    """plain-torch fp32 Swin block on zero-padded rows xp (B, H, W, Cp) with the padded parameter set P: heads are taken at stride hdp, the
    scale is the REAL head dim's"""
    B, H, W, Cp = xp.shape
    hd = C_ // heads
    h = _ln_real(xp, P["norm1_w"], P["norm1_b"], C_)
    if shift:
        h = torch.roll(h, (-shift, -shift), (1, 2))
    win = h.reshape(B, H // ws, ws, W // ws, ws, Cp).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, Cp)
    qkv = F.linear(win, P["qkv_w"], P["qkv_b"]).reshape(win.shape[0], ws * ws, 3, heads, hdp).permute(2, 0, 3, 1, 4)
    s = (qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5
    o = (torch.softmax(s, -1) @ qkv[2]).transpose(1, 2).reshape(-1, ws * ws, heads * hdp)
    o = F.linear(o, P["proj_w"], P["proj_b"])
    o = o.reshape(B, H // ws, W // ws, ws, ws, Cp).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, Cp)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    t = xp + o
    m = _ln_real(t, P["norm2_w"], P["norm2_b"], C_)
    m = F.linear(F.gelu(F.linear(m, P["fc1_w"], P["fc1_b"])), P["fc2_w"], P["fc2_b"])
    return t + m


def plain_block(x, blk, heads, ws, shift):
    """the unpadded block (B, H, W, C), the reference's arithmetic"""
    B, H, W, C_ = x.shape
    hd = C_ // heads
    a, m = blk.attn, blk.mlp
    h = F.layer_norm(x, (C_,), blk.norm1.weight, blk.norm1.bias, 1e-5)
    if shift:
        h = torch.roll(h, (-shift, -shift), (1, 2))
    win = h.reshape(B, H // ws, ws, W // ws, ws, C_).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C_)
    qkv = F.linear(win, a.qkv.weight, a.qkv.bias).reshape(win.shape[0], ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
    o = (torch.softmax((qkv[0] * hd ** -0.5) @ qkv[1].transpose(-2, -1), -1) @ qkv[2]).transpose(1, 2).reshape(-1, ws * ws, C_)
    o = F.linear(o, a.proj.weight, a.proj.bias)
    o = o.reshape(B, H // ws, W // ws, ws, ws, C_).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C_)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    t = x + o
    y = F.layer_norm(t, (C_,), blk.norm2.weight, blk.norm2.bias, 1e-5)
    return t + F.linear(F.gelu(F.linear(y, m.fc1.weight, m.fc1.bias)), m.fc2.weight, m.fc2.bias)


@pytest.mark.parametrize("C_,heads", [(180, 6), (36, 6), (60, 6), (64, 2)])
def test_padding_map(C_, heads):
    from basicsr.archs.swinir_arch import pad8, pad_block_params
    from dcpt_amd.keyed_init import keyed_input

    ws, shift, B, H, W = 4, 2, 2, 8, 12
    blk = _block(C_, heads, ws, shift, C_)
    P = pad_block_params(blk)
    hd = C_ // heads
    Cp, hdp = pad8(C_), pad8(hd)
    assert tuple(P["qkv_w"].shape) == (3 * heads * hdp, Cp) and tuple(P["proj_w"].shape) == (Cp, heads * hdp)
    assert all(v.dtype == torch.float32 for v in P.values())
    x = keyed_input(f"swpad{C_}.x", (B, H, W, C_), lo=-1.0, hi=1.0)
    xp = torch.zeros(B, H, W, Cp)
    xp[..., :C_] = x
    with torch.no_grad():
        want = plain_block(x, blk, heads, ws, shift)
        got = padded_block(xp, P, C_, heads, hdp, ws, shift)
    e = float((got[..., :C_] - want).abs().max() / want.abs().max())
    print(f"C={C_} heads={heads}: Cp={Cp} hdp={hdp}, real columns differ by {e:.3e} of the scale")
    assert e <= 2e-6   # fp32 rounding: the same sums with zeros added and the scale applied to the scores instead of q
    assert got[..., C_:].numel() == B * H * W * (Cp - C_)
    assert bool((got[..., C_:] == 0).all()), "pad columns must be exactly zero"
    # the placement itself: a permuted head order or a shifted row would not survive this
    q_rows = P["qkv_w"].reshape(3, heads, hdp, Cp)
    assert torch.equal(q_rows[:, :, :hd, :C_].reshape(3 * C_, C_), blk.attn.qkv.weight.detach())
    assert bool((q_rows[:, :, hd:, :] == 0).all()) and bool((q_rows[..., C_:] == 0).all())
    pw = P["proj_w"].reshape(Cp, heads, hdp)
    assert torch.equal(pw[:C_, :, :hd].reshape(C_, C_), blk.attn.proj.weight.detach())
    assert bool((pw[C_:] == 0).all()) and bool((pw[:, :, hd:] == 0).all())
