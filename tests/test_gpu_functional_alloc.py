"""Do the ops of dcpt_amd/functional.py still allocate through the three names tests/redzone.py swaps (``_workspace``, ``_empty_nhwc``,
``_empty_nhwc_bf16``)?  One forward + backward per op under the red zone at the smallest shape the op takes (B = 1, 4 x 4, C = 16; 8 x 8 in
bf16 storage; one window for Swin): something was guarded, the returned feature map starts one of the zone's allocations -- it came from
``_empty_nhwc*``, not from a private allocation the zone never sees -- and every guard is intact on exit (``redzone`` asserts that itself)."""
import pytest
import torch

from dcpt_amd import functional as DF
from dcpt_amd.keyed_init import keyed_input, keyed_tensor
from redzone import redzone

pytestmark = pytest.mark.gpu

B, C_, CR = 1, 16, 2
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _map(dev, tag, c, hw, bf=False, grad=True):
    x = keyed_input("alloc." + tag, (B, c, hw, hw), lo=-1.0, hi=1.0).to(dev).contiguous(memory_format=torch.channels_last)
    x = x.to(BF) if bf else x
    return x.requires_grad_(grad)


def _par(dev, tag, *shape):
    return keyed_tensor("alloc." + tag, shape).to(dev).requires_grad_(True)


def _conv(dev, tag, cout, cin, k):
    return _par(dev, tag + ".weight", cout, cin, k, k), _par(dev, tag + ".bias", cout)


def _ln(dev, tag, c):
    return (1.0 + _par(dev, tag + ".w", c).detach()).requires_grad_(True), _par(dev, tag + ".b", c)


# every case: name -> f(dev, bf) returning the op's feature map (or a tuple whose first entry it is)
def _layernorm2d(dev, bf):
    return DF.layernorm2d(_map(dev, "ln.x", C_, 4), *_ln(dev, "ln", C_))


def _conv3x3_in(dev, bf):
    hw = 8 if bf else 4
    img = keyed_input("alloc.in.x", (B, 3, hw, hw)).to(dev)
    return DF.conv3x3_in(img, *_conv(dev, "in", C_, 3, 3), out_bf16=bf)


def _down2x2(dev, bf):
    return DF.down2x2(_map(dev, "down.x", C_, 8 if bf else 4, bf), *_conv(dev, "down", 2 * C_, C_, 2))


def _down2x2_skip(dev, bf):
    return DF.down2x2_skip(_map(dev, "downs.x", C_, 8 if bf else 4, bf), *_conv(dev, "downs", 2 * C_, C_, 2))


def _up_ps(dev, bf):
    hw = 8 if bf else 4
    return DF.up_ps(_map(dev, "up.x", C_, hw, bf), _par(dev, "up.weight", 2 * C_, C_, 1, 1), _map(dev, "up.skip", C_ // 2, 2 * hw, bf))


def _conv_nobias(dev, bf):
    return DF.conv_nobias(_map(dev, "conv.x", C_, 8 if bf else 4, bf), _par(dev, "conv.weight", C_, C_, 3, 3))


def _pixel_shuffle2(dev, bf):
    return DF.pixel_shuffle2(_map(dev, "shuf.x", 2 * C_, 8 if bf else 4, bf))


def _concat_channels(dev, bf):
    hw = 8 if bf else 4
    return DF.concat_channels(_map(dev, "cat.a", C_, hw, bf), _map(dev, "cat.b", C_, hw, bf))


def _conv_ln(dev, bf):
    hw = 8 if bf else 4
    x, res = _map(dev, "cln.x", C_, hw, bf), _map(dev, "cln.res", C_, hw, bf)
    return (DF.conv_ln_bf16 if bf else DF.conv_ln)(x, _par(dev, "cln.weight", C_, C_, 3, 3), *_ln(dev, "cln", C_), res, True)


def _conv1x1_pool_relu(dev, bf):
    x = _map(dev, "pool.x", C_, 8 if bf else 4, bf)
    return (DF.conv1x1_pool_relu_bf16 if bf else DF.conv1x1_pool_relu)(x, _par(dev, "pool.weight", C_, C_, 1, 1))


def _mix(dev, bf):
    hw = 8 if bf else 4
    return DF.mix(_map(dev, "mix.prev", C_, hw, bf), _map(dev, "mix.feat", C_, hw, bf), _par(dev, "mix.w", 4), 1)


def _mdta(dev, bf):
    x = _map(dev, "mdta.x", C_, 8 if bf else 4, bf)
    nw, nb = _ln(dev, "mdta", C_)
    return DF.mdta(x, nw, nb, _par(dev, "mdta.qkv", 3 * C_, C_, 1, 1), _par(dev, "mdta.dw", 3 * C_, 1, 3, 3), _par(dev, "mdta.proj", C_, C_, 1, 1),
                   (1.0 + _par(dev, "mdta.temp", 2, 1, 1).detach()).requires_grad_(True), 2, False)


def _gdfn(dev, bf):
    x = _map(dev, "gdfn.x", C_, 8 if bf else 4, bf)
    nw, nb = _ln(dev, "gdfn", C_)
    hid = 2 * C_
    return DF.gdfn(x, nw, nb, _par(dev, "gdfn.in", 2 * hid, C_, 1, 1), _par(dev, "gdfn.dw", 2 * hid, 1, 3, 3), _par(dev, "gdfn.out", C_, hid, 1, 1), False)


def _prompt_mix(dev, bf):
    hw = 8 if bf else 4
    return DF.prompt_mix(_par(dev, "pm.logits", B, 5), _par(dev, "pm.param", 1, 5, C_, 4, 4), hw, hw, out_bf16=bf)


def _swin_attn(dev, bf):
    nw, nb = _ln(dev, "swa", C_)
    return DF.swin_attn(_map(dev, "swa.x", C_, 4), nw, nb, _par(dev, "swa.qkv_w", 3 * C_, C_), _par(dev, "swa.qkv_b", 3 * C_),
                        _par(dev, "swa.proj_w", C_, C_), _par(dev, "swa.proj_b", C_), 2, 4, 0)


def _swin_mlp(dev, bf):
    nw, nb = _ln(dev, "swm", C_)
    return DF.swin_mlp(_map(dev, "swm.x", C_, 4), nw, nb, _par(dev, "swm.fc1_w", 2 * C_, C_), _par(dev, "swm.fc1_b", 2 * C_),
                       _par(dev, "swm.fc2_w", C_, 2 * C_), _par(dev, "swm.fc2_b", C_))


def _conv3x3_res(dev, bf):
    return DF.conv3x3_res(_map(dev, "c3r.x", C_, 4), *_conv(dev, "c3r", C_, C_, 3), _map(dev, "c3r.res", C_, 4))


def _rcab_params(dev):
    return (*_conv(dev, "rcab.c1", C_, C_, 3), *_conv(dev, "rcab.c2", C_, C_, 3), *_conv(dev, "rcab.ca1", CR, C_, 1), *_conv(dev, "rcab.ca2", C_, CR, 1))


def _rcab(dev, bf):
    return DF.rcab(_map(dev, "rcab.x", C_, 4), *_rcab_params(dev), res_scale=1.0)


def _conv3x3_ps(dev, bf):
    return DF.conv3x3_ps(_map(dev, "ps.x", C_, 4), *_conv(dev, "ps", 4 * C_, C_, 3), 2)


def _conv3x3_act(dev, bf):
    return DF.conv3x3_act(_map(dev, "act.x", C_, 4), *_conv(dev, "act", C_, C_, 3), 0.2)


def _up2_conv3x3_act(dev, bf):
    return DF.up2_conv3x3_act(_map(dev, "up2.x", C_, 4), *_conv(dev, "up2", C_, C_, 3), 0.2)


def _conv3conv_res(dev, bf):
    q = C_ // 4
    return DF.conv3conv_res(_map(dev, "3c.x", C_, 4), *_conv(dev, "3c.1", q, C_, 3), *_conv(dev, "3c.2", q, q, 1), *_conv(dev, "3c.3", C_, q, 3),
                            _map(dev, "3c.res", C_, 4))


# forward only (bf16 storage for RCAN is inference-only): called under torch.no_grad()
def _rcab_bf16(dev, bf):
    return DF.rcab_bf16(_map(dev, "rcab16.x", C_, 8, True, grad=False), *_rcab_params(dev), res_scale=1.0)


def _conv3x3_res_bf16(dev, bf):
    return DF.conv3x3_res_bf16(_map(dev, "c3r16.x", C_, 8, True, grad=False), *_conv(dev, "c3r16", C_, C_, 3), _map(dev, "c3r16.res", C_, 8, True, grad=False))


def _conv3x3_ps_bf16(dev, bf):
    return DF.conv3x3_ps_bf16(_map(dev, "ps16.x", C_, 8, True, grad=False), *_conv(dev, "ps16", 4 * C_, C_, 3), 2)


_BOTH = [_conv3x3_in, _down2x2, _down2x2_skip, _up_ps, _conv_nobias, _pixel_shuffle2, _concat_channels, _conv_ln, _conv1x1_pool_relu, _mix,
         _mdta, _gdfn, _prompt_mix]
_FP32 = [_layernorm2d, _swin_attn, _swin_mlp, _conv3x3_res, _rcab, _conv3x3_ps, _conv3x3_act, _up2_conv3x3_act, _conv3conv_res]
_FWD_BF16 = [_rcab_bf16, _conv3x3_res_bf16, _conv3x3_ps_bf16]
CASES = ([(f, False, True) for f in _BOTH + _FP32] + [(f, True, True) for f in _BOTH] + [(f, True, False) for f in _FWD_BF16])


@pytest.mark.parametrize("op,bf,backward", CASES, ids=[f"{f.__name__[1:]}-{'bf16' if bf else 'fp32'}" for f, bf, _ in CASES])
def test_outputs_come_from_the_guarded_allocators(dev, op, bf, backward):
    with redzone() as rz:
        if backward:
            out = op(dev, bf)
            y = out[0] if isinstance(out, tuple) else out
            y.float().sum().backward()
        else:
            with torch.no_grad():
                y = op(dev, bf)
        starts = {raw.data_ptr() for _, raw, _ in rz.allocs}
    assert rz.count > 0, "nothing was allocated through the patched helpers: the red zone checked nothing"
    assert y.dtype == (BF if bf else torch.float32)
    assert y.data_ptr() in starts, f"the result of {op.__name__[1:]} was not allocated by _empty_nhwc / _empty_nhwc_bf16"
