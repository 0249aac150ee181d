"""act_dtype="bf16_res32" (RCAN / SwinIR on bf16 maps around an fp32 residual stream), the parts that need no GPU: the public surface accepts
the mode and refuses what "bf16" refuses, the state_dict does not depend on it, the inference-only checks come first, the new entry points
are in the header, in ``_lib.SIGNATURES`` and in the library at ABI 16, their workspace queries need no device, and bad arguments are refused
before anything is touched."""
import ctypes as C
import os
import re

import pytest
import torch

MODE = "bf16_res32"
SWIN = dict(embed_dim=36, depths=[2] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
RCAN = dict(num_in_ch=3, num_out_ch=3, num_feat=32, num_group=2, num_block=2, upscale=2)
NEW_NAMES = ("dcpt_rcab_bf16_res32_ws_bytes", "dcpt_rcab_fwd_bf16_res32", "dcpt_conv3x3_res_bf16_res32_ws_bytes", "dcpt_conv3x3_res_fwd_bf16_res32",
             "dcpt_ln_pad_fwd_bf16_res32", "dcpt_swin_attn_bf16_res32_ws_bytes", "dcpt_swin_attn_fwd_bf16_res32", "dcpt_swin_mlp_bf16_res32_ws_bytes",
             "dcpt_swin_mlp_fwd_bf16_res32")


@pytest.fixture(scope="module")
def lib():
    from dcpt_amd import _lib

    return _lib.load()


def _swin(**kw):
    from basicsr.archs import build_network

    return build_network(dict(type="SwinIR", **dict(SWIN, **kw)))


def _rcan(**kw):
    from basicsr.archs import build_network

    return build_network(dict(type="RCAN", **dict(RCAN, **kw)))


# ---- public surface ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [_swin, _rcan])
def test_mode_is_accepted_everywhere(build):
    assert build(act_dtype=MODE).act_dtype == MODE       # constructor = the options spelling network_g.act_dtype
    net = build()
    assert net.act_dtype == "fp32"
    for act in (MODE, "bf16", MODE, "fp32"):
        net.set_act_dtype(act)
        assert net.act_dtype == act
    for bad in ("fp16", "bf16_res", "res32", ""):
        with pytest.raises(ValueError, match="act_dtype"):
            net.set_act_dtype(bad)
        with pytest.raises(ValueError, match="act_dtype"):
            build(act_dtype=bad)
    assert net.act_dtype == "fp32"


def test_srmodel_options_spelling():
    from basicsr.models import build_model

    for net_g in (dict(type="SwinIR", **SWIN), dict(type="RCAN", **RCAN)):
        opt = dict(name="t", model_type="SRModel", scale=net_g["upscale"], num_gpu=0, dist=False, rank=0, world_size=1, is_train=False,
                   network_g=dict(net_g, act_dtype=MODE), path=dict(pretrain_network_g=None), val=dict(save_img=False))
        assert build_model(opt).net_g.act_dtype == MODE


def test_rcan_refuses_what_bf16_refuses():
    with pytest.raises(ValueError, match="num_feat % 8"):
        _rcan(num_feat=12, squeeze_factor=4, act_dtype=MODE)
    net = _rcan(num_feat=12, squeeze_factor=4)
    for act in ("bf16", MODE):
        with pytest.raises(ValueError, match="num_feat % 8"):
            net.set_act_dtype(act)
    assert net.act_dtype == "fp32"


@pytest.mark.parametrize("kw,what", [(dict(upsampler="pixelshuffle", upscale=2), "upsampler"), (dict(upsampler="pixelshuffledirect", upscale=3), "upsampler"),
                                     (dict(upsampler="nearest+conv", upscale=4), "upsampler"), (dict(embed_dim=48, resi_connection="3conv"), "3conv"),
                                     (dict(embed_dim=264), "256"), (dict(mlp_ratio=1.0), "multiple of 8")])
def test_swinir_refuses_what_bf16_refuses(kw, what):
    with pytest.raises(NotImplementedError, match=what):
        _swin(act_dtype=MODE, **kw)
    net = _swin(**kw)
    for act in ("bf16", MODE):
        with pytest.raises(NotImplementedError, match=what):
            net.set_act_dtype(act)
    assert net.act_dtype == "fp32"


def test_widest_padded_width_is_taken():
    net = _swin(embed_dim=252)
    net.set_act_dtype(MODE)
    assert net.padded_dim() == 256


@pytest.mark.parametrize("build,nkeys", [(_swin, 166), (_rcan, None)])
def test_state_dict_does_not_depend_on_the_mode(build, nkeys):
    a, b, c = build(), build(act_dtype="bf16"), build(act_dtype=MODE)
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert list(sa.keys()) == list(sb.keys()) == list(sc.keys()) and (nkeys is None or len(sc) == nkeys)
    assert all(sa[k].shape == sc[k].shape and sc[k].dtype == torch.float32 for k in sa)
    assert all(p.dtype == torch.float32 for p in c.parameters())
    c.load_state_dict(sa, strict=True)


def test_swinir_operand_caches_are_shared_between_the_bf16_modes():
    net = _swin(act_dtype="bf16")
    blk = net.encode_layers[0].residual_group.blocks[0]
    assert blk.refresh_bf16() is True
    pack = blk._swin_bf16
    net.set_act_dtype(MODE)
    assert blk.refresh_bf16() is False and blk._swin_bf16 is pack   # the same cached operands serve both modes


@pytest.mark.parametrize("build", [_swin, _rcan])
def test_inference_only_is_checked_before_anything_runs(build):
    net = build(act_dtype=MODE)
    with pytest.raises(NotImplementedError, match="inference-only"):
        net(torch.zeros(1, 3, 8, 8))                                   # parameters require grad, grad mode on
    net.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="inference-only"):
        net(torch.zeros(1, 3, 8, 8, requires_grad=True))               # the input requires grad
    if build is _swin:
        with torch.no_grad():
            with pytest.raises(NotImplementedError, match="inference-only"):
                net(torch.zeros(1, 3, 8, 8), hook=True)                # the tap pass belongs to training


@pytest.mark.parametrize("build", [_swin, _rcan])
def test_cpu_tensors_raise(lib, build):
    from dcpt_amd._lib import DcptHipError

    net = build(act_dtype=MODE)
    with torch.no_grad():
        with pytest.raises(DcptHipError):
            net(torch.zeros(1, 3, 8, 8))


def test_functional_wrappers_refuse_cpu_tensors(lib):
    from dcpt_amd import functional as DF
    from dcpt_amd._lib import DcptHipError

    s, sb = torch.zeros(1, 40, 8, 8), torch.zeros(1, 40, 8, 8, dtype=torch.bfloat16)
    w, b = torch.zeros(40, 40, 3, 3), torch.zeros(40)
    with torch.no_grad():
        with pytest.raises(DcptHipError):
            DF.ln_pad_bf16_res32(s, torch.zeros(40), torch.zeros(40), 36)
        with pytest.raises(DcptHipError):
            DF.conv3x3_res_bf16_res32(sb, w, b, s)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_names_in_header_signatures_and_library_at_abi_16(lib):
    from dcpt_amd import _lib

    assert lib.dcpt_abi_version() == _lib.ABI_VERSION == 16
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dcpt_hip.h")).read()
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), f"{name} is not declared in include/dcpt_hip.h"


def test_ws_queries_need_no_device(lib):
    rcab, res = lib.dcpt_rcab_bf16_res32_ws_bytes, lib.dcpt_conv3x3_res_bf16_res32_ws_bytes
    att, mlp = lib.dcpt_swin_attn_bf16_res32_ws_bytes, lib.dcpt_swin_mlp_bf16_res32_ws_bytes
    # (B, H, W, C, Cr) / (B, H, W, C) / (B, H, W, C, Cp, heads, hdp, window) / (B, H, W, C, Cp, hidden)
    assert rcab(2, 13, 17, 64, 4) > 0 and rcab(1, 256, 256, 64, 4) > 0 and res(2, 13, 17, 64) > 0 and res(1, 8, 8, 184) > 0
    assert att(2, 16, 24, 180, 184, 6, 32, 8) > 0 and att(3, 8, 8, 36, 40, 6, 8, 8) > 0
    assert mlp(2, 16, 24, 180, 184, 360) > 0 and mlp(3, 8, 8, 36, 40, 72) > 0
    assert rcab(2, 13, 17, 60, 4) == 0 and rcab(2, 13, 17, 64, 0) == 0 and rcab(0, 13, 17, 64, 4) == 0 and rcab(1, 8, 8, 2048, 4) == 0
    assert res(2, 13, 17, 60) == 0 and res(2, 0, 17, 64) == 0
    assert att(2, 16, 24, 180, 180, 6, 32, 8) == 0    # Cp % 8
    assert att(2, 16, 24, 180, 184, 6, 24, 8) == 0    # hdp < hd
    assert att(2, 18, 27, 180, 184, 6, 32, 9) == 0    # ws^2 > 64
    assert att(2, 16, 20, 180, 184, 6, 32, 8) == 0    # W % ws
    assert att(2, 16, 24, 180, 264, 6, 32, 8) == 0    # Cp > 256
    assert mlp(2, 16, 24, 180, 176, 360) == 0         # C > Cp
    assert mlp(2, 16, 24, 180, 184, 364) == 0         # hidden % 8
    # the stream form keeps the bf16 form's intermediates
    assert rcab(2, 13, 17, 64, 4) == lib.dcpt_rcab_bf16_ws_bytes(2, 13, 17, 64, 4)
    assert att(3, 8, 8, 36, 40, 6, 8, 8) == lib.dcpt_swin_attn_bf16_ws_bytes(3, 8, 8, 36, 40, 6, 8, 8)


def test_bad_arguments_return_an_error_instead_of_crashing(lib):
    from dcpt_amd._lib import RcabParams, SwinAttnBf16Params, SwinMlpBf16Params

    # host memory stands in for device buffers: every call below must be refused before it touches them
    buf = (C.c_char * (1 << 16))()
    p = C.addressof(buf)

    def refused(rc, what):
        assert rc != 0
        msg = lib.dcpt_last_error().decode()
        assert what in msg, msg

    geo = (1, 8, 8, 36, 40, 6, 8, 8)
    pa, pm = SwinAttnBf16Params(p, p, p, p, p, p), SwinMlpBf16Params(p, p, p, p, p, p)
    need = lib.dcpt_swin_attn_bf16_res32_ws_bytes(*geo)
    att = lib.dcpt_swin_attn_fwd_bf16_res32
    refused(att(None, p, p, p, need, *geo, 0, None), "null")
    refused(att(C.byref(pa), None, p, p, need, *geo, 0, None), "null")
    refused(att(C.byref(pa), p, None, p, need, *geo, 0, None), "null")
    refused(att(C.byref(SwinAttnBf16Params(p, p, p, p, None, p)), p, p, p, need, *geo, 0, None), "null")
    refused(att(C.byref(pa), p, p, p, need, 1, 8, 8, 36, 36, 6, 8, 8, 0, None), "Cp a multiple of 8")
    refused(att(C.byref(pa), p, p, p, need, *geo, 8, None), "shift")
    refused(att(C.byref(pa), p, p, p, need - 1, *geo, 0, None), "workspace too small")
    refused(att(C.byref(pa), p, p, None, need, *geo, 0, None), "workspace too small")

    mgeo = (1, 8, 8, 36, 40, 72)
    need = lib.dcpt_swin_mlp_bf16_res32_ws_bytes(*mgeo)
    mlp = lib.dcpt_swin_mlp_fwd_bf16_res32
    refused(mlp(None, p, p, p, p, need, *mgeo, None), "null")
    refused(mlp(C.byref(pm), None, p, None, p, need, *mgeo, None), "null")
    refused(mlp(C.byref(pm), p, None, p, p, need, *mgeo, None), "null")          # the fp32 output is not optional
    refused(mlp(C.byref(pm), p, p, None, p, need, 1, 8, 8, 36, 40, 36, None), "hidden")
    refused(mlp(C.byref(pm), p, p, None, p, need - 1, *mgeo, None), "workspace too small")

    ln = lib.dcpt_ln_pad_fwd_bf16_res32
    refused(ln(None, p, p, p, 64, 36, 40, 1e-5, None), "null")
    refused(ln(p, p, p, None, 64, 36, 40, 1e-5, None), "null")
    refused(ln(p, p, p, p, 64, 36, 36, 1e-5, None), "multiple of 8")
    refused(ln(p, p, p, p, 64, 44, 40, 1e-5, None), "C <= Cp")
    refused(ln(p, p, p, p, 0, 36, 40, 1e-5, None), "M=0")

    rgeo = (2, 13, 17, 64, 4)
    pr = RcabParams(p, p, p, p, p, p, p, p)
    need = lib.dcpt_rcab_bf16_res32_ws_bytes(*rgeo)
    rcab = lib.dcpt_rcab_fwd_bf16_res32
    refused(rcab(None, None, 0, None, 0, p, p, p, p, p, need, *rgeo, 1.0, None), "null")
    for hole in range(4):   # the stream, its image and both outputs are all required
        maps = [p, p, p, p]
        maps[hole] = None
        refused(rcab(C.byref(pr), None, 0, None, 0, *maps, p, need, *rgeo, 1.0, None), "null")
    refused(rcab(C.byref(RcabParams(None, p, p, p, p, p, p, p)), None, 0, None, 0, p, p, p, p, p, need, *rgeo, 1.0, None), "null")
    refused(rcab(C.byref(pr), None, 0, None, 0, p, p, p, p, p, need, 2, 13, 17, 60, 4, 1.0, None), "multiple of 8")
    refused(rcab(C.byref(pr), p, 16, None, 0, p, p, p, p, p, need, *rgeo, 1.0, None), "packed weights too small")
    refused(rcab(C.byref(pr), None, 0, None, 0, p, p, p, p, p, need - 1, *rgeo, 1.0, None), "workspace too small")

    cgeo = (2, 13, 17, 64)
    need = lib.dcpt_conv3x3_res_bf16_res32_ws_bytes(*cgeo)
    res = lib.dcpt_conv3x3_res_fwd_bf16_res32
    refused(res(None, p, None, 0, p, p, p, p, p, need, *cgeo, None), "null")
    refused(res(p, p, None, 0, p, None, p, p, p, need, *cgeo, None), "null")      # no residual
    refused(res(p, p, None, 0, p, p, None, None, p, need, *cgeo, None), "null")   # neither output
    refused(res(p, None, None, 0, p, p, p, p, p, need, *cgeo, None), "null")      # neither weights nor a pack
    refused(res(p, p, None, 0, p, p, p, p, p, need, 2, 13, 17, 60, None), "multiple of 8")
    refused(res(p, p, None, 0, p, p, p, None, p, need - 1, *cgeo, None), "workspace too small")
    assert bytes(buf) == bytes(len(buf)), "a refused call wrote into its buffers"
