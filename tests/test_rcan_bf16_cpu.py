"""RCAN on bf16 activation storage, the parts that need no GPU: constructor validation, state_dict keys, the device-free workspace queries
and the argument checks of dcpt_rcab_fwd_bf16 / dcpt_conv3x3_res_fwd_bf16 / dcpt_conv3x3_ps_fwd_bf16 (refused before any launch)."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from dcpt_amd import _lib

    return _lib.load()


def _build(**kw):
    from basicsr.archs import build_network

    return build_network(dict(type="RCAN", num_in_ch=3, num_out_ch=3, **kw))


def test_constructor_validation():
    with pytest.raises(ValueError, match="act_dtype"):
        _build(act_dtype="fp16")
    with pytest.raises(ValueError, match="num_feat % 8"):
        _build(num_feat=36, squeeze_factor=4, num_group=1, num_block=1, act_dtype="bf16")
    net = _build(num_feat=36, squeeze_factor=4, num_group=1, num_block=1)   # fp32 takes a multiple of 4
    assert net.act_dtype == "fp32"
    with pytest.raises(ValueError, match="num_feat % 8"):
        net.set_act_dtype("bf16")
    with pytest.raises(ValueError, match="act_dtype"):
        net.set_act_dtype("half")
    assert net.act_dtype == "fp32"


def test_state_dict_keys_do_not_depend_on_act_dtype():
    a, b = _build(), _build(act_dtype="bf16")
    assert b.act_dtype == "bf16"
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys()) and len(sb) == 1310
    assert all(sa[k].shape == sb[k].shape and sb[k].dtype == torch.float32 for k in sa)
    b.set_act_dtype("fp32")
    b.set_act_dtype("bf16")
    assert list(b.state_dict().keys()) == list(sa.keys())
    assert len(b._convs_bf16()) == 333   # one cached operand image per 3 x 3 conv of the body and the tail
    assert list(b.state_dict().keys()) == list(sa.keys())   # (the caches are plain attributes)


def test_inference_only_is_checked_before_anything_runs():
    net = _build(num_feat=16, squeeze_factor=4, num_group=1, num_block=1, act_dtype="bf16")
    with pytest.raises(NotImplementedError, match="inference-only"):
        net(torch.zeros(1, 3, 8, 8))


def test_ws_queries_need_no_device(lib):
    assert lib.dcpt_rcab_bf16_ws_bytes(2, 13, 17, 64, 4) > 0
    assert lib.dcpt_conv3x3_res_bf16_ws_bytes(2, 13, 17, 64) > 0
    assert lib.dcpt_conv3x3_ps_bf16_ws_bytes(2, 13, 17, 64, 2) > 0
    assert lib.dcpt_conv3x3_ps_bf16_ws_bytes(2, 13, 17, 64, 3) > 0
    # C % 8 != 0, r not in {2, 3}, Cr out of range, empty maps
    assert lib.dcpt_rcab_bf16_ws_bytes(2, 13, 17, 36, 4) == 0
    assert lib.dcpt_rcab_bf16_ws_bytes(2, 13, 17, 64, 0) == 0
    assert lib.dcpt_rcab_bf16_ws_bytes(2, 13, 17, 64, 65) == 0
    assert lib.dcpt_rcab_bf16_ws_bytes(0, 13, 17, 64, 4) == 0
    assert lib.dcpt_conv3x3_res_bf16_ws_bytes(2, 13, 17, 12) == 0
    assert lib.dcpt_conv3x3_ps_bf16_ws_bytes(2, 13, 17, 36, 2) == 0
    for r in (0, 1, 4, 5):
        assert lib.dcpt_conv3x3_ps_bf16_ws_bytes(2, 13, 17, 64, r) == 0


def test_bad_arguments_return_an_error_instead_of_crashing(lib):
    from dcpt_amd._lib import RcabParams

    B, H, W, Cc, Cr = 1, 4, 4, 8, 2
    # host memory stands in for device buffers: every call below must be refused before it touches them
    buf = (C.c_char * (1 << 16))()
    p = C.addressof(buf)
    pp = RcabParams(p, p, p, p, p, p, p, p)
    need = lib.dcpt_rcab_bf16_ws_bytes(B, H, W, Cc, Cr)

    def refused(rc, what):
        assert rc != 0
        msg = lib.dcpt_last_error().decode()
        assert what in msg, msg

    refused(lib.dcpt_rcab_fwd_bf16(None, None, 0, None, 0, p, p, p, need, B, H, W, Cc, Cr, 1.0, None), "null")
    refused(lib.dcpt_rcab_fwd_bf16(C.byref(pp), None, 0, None, 0, None, p, p, need, B, H, W, Cc, Cr, 1.0, None), "null")
    refused(lib.dcpt_rcab_fwd_bf16(C.byref(RcabParams(None, p, p, p, p, p, p, p)), None, 0, None, 0, p, p, p, need, B, H, W, Cc, Cr, 1.0, None), "null")
    refused(lib.dcpt_rcab_fwd_bf16(C.byref(pp), None, 0, None, 0, p, p, p, need, B, H, W, 12, Cr, 1.0, None), "multiple of 8")
    refused(lib.dcpt_rcab_fwd_bf16(C.byref(pp), None, 0, None, 0, p, p, p, need - 1, B, H, W, Cc, Cr, 1.0, None), "workspace too small")
    refused(lib.dcpt_rcab_fwd_bf16(C.byref(pp), None, 0, None, 0, p, p, None, need, B, H, W, Cc, Cr, 1.0, None), "workspace too small")
    refused(lib.dcpt_rcab_fwd_bf16(C.byref(pp), p, 16, None, 0, p, p, p, need, B, H, W, Cc, Cr, 1.0, None), "packed weights too small")

    need = lib.dcpt_conv3x3_res_bf16_ws_bytes(B, H, W, Cc)
    refused(lib.dcpt_conv3x3_res_fwd_bf16(p, p, None, 0, p, None, p, p, need, B, H, W, Cc, None), "null")
    refused(lib.dcpt_conv3x3_res_fwd_bf16(p, None, None, 0, p, p, p, p, need, B, H, W, Cc, None), "null")
    refused(lib.dcpt_conv3x3_res_fwd_bf16(p, p, None, 0, p, p, p, p, need, B, H, W, 20, None), "multiple of 8")
    refused(lib.dcpt_conv3x3_res_fwd_bf16(p, p, None, 0, p, p, p, p, need - 1, B, H, W, Cc, None), "workspace too small")

    need = lib.dcpt_conv3x3_ps_bf16_ws_bytes(B, H, W, Cc, 3)
    refused(lib.dcpt_conv3x3_ps_fwd_bf16(None, p, None, 0, p, p, p, need, B, H, W, Cc, 3, None), "null")
    refused(lib.dcpt_conv3x3_ps_fwd_bf16(p, p, None, 0, p, p, p, need, B, H, W, Cc, 4, None), "r 2 or 3")
    refused(lib.dcpt_conv3x3_ps_fwd_bf16(p, p, None, 0, p, p, p, need, B, H, W, 12, 2, None), "multiple of 8")
    refused(lib.dcpt_conv3x3_ps_fwd_bf16(p, p, None, 0, p, p, p, need - 1, B, H, W, Cc, 3, None), "workspace too small")


def test_cpu_tensors_raise(lib):
    from dcpt_amd import functional as DF
    from dcpt_amd._lib import DcptHipError

    x = torch.zeros(1, 8, 4, 4, dtype=torch.bfloat16)
    w, b = torch.zeros(8, 8, 3, 3), torch.zeros(8)
    with torch.no_grad():
        with pytest.raises(DcptHipError):
            DF.rcab_bf16(x, w, b, w, b, torch.zeros(2, 8, 1, 1), torch.zeros(2), torch.zeros(8, 2, 1, 1), b)
        with pytest.raises(DcptHipError):
            DF.conv3x3_res_bf16(x, w, b, x)
        with pytest.raises(DcptHipError):
            DF.conv3x3_ps_bf16(x, torch.zeros(32, 8, 3, 3), torch.zeros(32), 2)
        net = _build(num_feat=16, squeeze_factor=4, num_group=1, num_block=1, act_dtype="bf16")
        with pytest.raises(DcptHipError):
            net(torch.zeros(1, 3, 8, 8))


def test_abi_version_unchanged(lib):
    from dcpt_amd import _lib

    assert lib.dcpt_abi_version() == _lib.ABI_VERSION == 16
    for name in ("dcpt_rcab_bf16_ws_bytes", "dcpt_rcab_fwd_bf16", "dcpt_conv3x3_res_bf16_ws_bytes", "dcpt_conv3x3_res_fwd_bf16",
                 "dcpt_conv3x3_ps_bf16_ws_bytes", "dcpt_conv3x3_ps_fwd_bf16"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
