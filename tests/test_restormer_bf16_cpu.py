"""CPU: Restormer act_dtype="bf16" construction, argument checks and the new C entry points' argument errors (no GPU needed)."""
import ctypes as C

import pytest
import torch

from basicsr.archs import build_network
from dcpt_amd import _lib

R_CFG = dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, heads=[1, 2, 4, 8])


@pytest.mark.parametrize("name", ["Restormer", "Restormer_origin"])
def test_bf16_build_same_state_dict(name):
    a = build_network(dict(type=name, **R_CFG))
    b = build_network(dict(type=name, act_dtype="bf16", **R_CFG))
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert all(sa[k].shape == sb[k].shape and sb[k].dtype == torch.float32 for k in sa)
    assert a.act_dtype == "fp32" and b.act_dtype == "bf16"


@pytest.mark.parametrize("name", ["Restormer", "Restormer_origin"])
def test_bad_act_dtype(name):
    with pytest.raises(ValueError):
        build_network(dict(type=name, act_dtype="fp16", **R_CFG))


def test_cpu_tensor_raises():
    net = build_network(dict(type="Restormer", act_dtype="bf16", **R_CFG))
    with pytest.raises(_lib.DcptHipError):
        net(torch.rand(1, 3, 16, 16))


def test_ws_queries_without_gpu():
    lib = _lib.load()
    assert lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 48, 1, 0) > 0
    assert lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 48, 1, 1) > lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 48, 1, 0)
    assert lib.dcpt_gdfn_bf16_ws_bytes(2, 16, 16, 48, 127, 1) > 0
    assert lib.dcpt_conv_bf16_ws_bytes(2, 16, 16, 48, 24, 3, 1) > 0
    # full save mode (every optional saved tensor supplied by the caller): no workspace copies of them
    for bwd in (0, 1):
        assert 0 < lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 48, 1, bwd | 2) < lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 48, 1, bwd)
        assert 0 < lib.dcpt_gdfn_bf16_ws_bytes(2, 16, 16, 48, 127, bwd | 2) < lib.dcpt_gdfn_bf16_ws_bytes(2, 16, 16, 48, 127, bwd)
    # shapes the entry points reject answer 0
    assert lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 48, 5, 0) == 0      # C % heads
    assert lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 48, 12, 0) == 0     # head width 4
    assert lib.dcpt_gdfn_bf16_ws_bytes(2, 16, 16, 48, 0, 0) == 0      # hidden
    assert lib.dcpt_abi_version() == 16


def _err(rc):
    assert rc != 0
    return _lib.load().dcpt_last_error().decode()


def test_argument_errors_reported():
    lib = _lib.load()
    pp, gg = _lib.MdtaParams(), _lib.MdtaParams()
    sv = _lib.MdtaSaved()
    assert "null" in _err(lib.dcpt_mdta_bf16_fwd(C.byref(pp), None, None, C.byref(sv), None, 0, 1, 4, 4, 48, 1, 1, None))
    assert "null" in _err(lib.dcpt_mdta_bf16_bwd(C.byref(pp), C.byref(gg), None, C.byref(sv), None, None, None, 0, 1, 4, 4, 48, 1, 1, None))
    # non-null dummies (never dereferenced: the shape checks come first)
    fake = 256
    full = _lib.MdtaParams(*([fake] * 6))
    fsv = _lib.MdtaSaved(*([fake] * 10))
    assert "heads" in _err(lib.dcpt_mdta_bf16_fwd(C.byref(full), fake, fake, C.byref(fsv), None, 0, 1, 4, 4, 48, 5, 1, None))
    assert "heads" in _err(lib.dcpt_mdta_bf16_fwd(C.byref(full), fake, fake, C.byref(fsv), None, 0, 1, 4, 4, 48, 12, 1, None))
    gp = _lib.GdfnParams(*([fake] * 5))
    gs = _lib.GdfnSaved(*([fake] * 5))
    assert "hidden" in _err(lib.dcpt_gdfn_bf16_fwd(C.byref(gp), fake, fake, C.byref(gs), None, 0, 1, 4, 4, 48, 0, 1, None))
    assert "null" in _err(lib.dcpt_gdfn_bf16_fwd(C.byref(gp), None, fake, C.byref(gs), None, 0, 1, 4, 4, 48, 127, 1, None))
    assert "bad argument" in _err(lib.dcpt_concat_channels_bf16(fake, fake, fake, 4, 4, 8, None))
    assert "bad argument" in _err(lib.dcpt_pixel_unshuffle_bf16(fake, fake, 1, 5, 4, 8, None))
    assert "Cin" in _err(lib.dcpt_conv_fwd_bf16(fake, fake, fake, None, 0, 1, 4, 4, 12, 8, 3, None))
