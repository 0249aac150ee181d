"""The fp32 SwinIR / SwinIR-SR / RCAN / classifier-head entry points refuse a short or null workspace (DCPT_ERR_WS, "workspace too small"
and the op's name in the message), a null operand and the shapes their queries refuse (DCPT_ERR_ARG) -- all before any launch, so no GPU is
needed: a host buffer stands in for device memory."""
import ctypes as C

import pytest

ERR_ARG, ERR_WS = 1, 2
B, H, W, CH = 1, 4, 4, 16


@pytest.fixture(scope="module")
def lib():
    from dcpt_amd import _lib

    return _lib.load()


_buf = (C.c_char * (1 << 16))()
P = C.addressof(_buf)


def _struct(cls):
    return C.byref(cls(*([P] * len(cls._fields_))))


def _ops():
    """(name, query arguments without the backward flag, forward head, backward head, arguments after ws_bytes): the heads are the
    pointer (and flag) arguments in front of ws; the first of them is a required operand of every op."""
    from dcpt_amd._lib import Conv3convParams, RcabParams, RcabSaved, SwinAttnParams, SwinAttnSaved, SwinMlpParams, SwinMlpSaved

    s = _struct
    return [
        ("swin_attn", (B, H, W, CH, 2), [s(SwinAttnParams), P, P, s(SwinAttnSaved)],
         [s(SwinAttnParams), s(SwinAttnParams), P, s(SwinAttnSaved), P, P], (B, H, W, CH, 2, 4, 0)),
        ("swin_mlp", (B, H, W, CH, 32), [s(SwinMlpParams), P, P, s(SwinMlpSaved)],
         [s(SwinMlpParams), s(SwinMlpParams), P, s(SwinMlpSaved), P, P], (B, H, W, CH, 32)),
        ("conv3x3_res", (B, H, W, CH), [P] * 5, [P] * 6, (B, H, W, CH)),
        ("conv3x3_act", (B, H, W, CH, CH), [P] * 4, [P] * 7, (B, H, W, CH, CH, 0.2)),
        ("up2_conv3x3_act", (B, H, W, CH), [P] * 4, [P] * 7, (B, H, W, CH, 0.2)),
        ("conv3x3_ps_out", (B, H, W, CH, 3, 3), [P] * 4, [P] * 6, (B, H, W, CH, 3, 3)),
        ("conv3conv_res", (B, H, W, CH), [s(Conv3convParams), P, P, P, P, P],
         [s(Conv3convParams), s(Conv3convParams), P, P, P, P, P], (B, H, W, CH)),
        ("rcab", (B, H, W, CH, 2), [s(RcabParams), P, P, s(RcabSaved)], [s(RcabParams), s(RcabParams), P, s(RcabSaved), P, P],
         (B, H, W, CH, 2, 1.0)),
        ("conv3x3_ps", (B, H, W, CH, 2), [P] * 4, [P] * 6, (B, H, W, CH, 2)),
        ("conv", (B, H, W, CH, CH, 3), [P] * 3, [P] * 5, (B, H, W, CH, CH, 3)),
        ("conv", (B, H, W, CH, CH, 1), [P] * 3, [P] * 5, (B, H, W, CH, CH, 1)),
        # conv_ln_fwd(x, w, lnw, lnb, res, relu, z, y, mu, rstd, ...);  conv_ln_bwd(dy, x, w, lnw, z, y, mu, rstd, dx_add = NULL, dx, dw,
        # dlnw, dlnb, dres, ..., relu)
        ("conv_ln", (B, H, W, CH, CH, 3), [P, P, P, P, P, 1, P, P, P, P], [P] * 8 + [None] + [P] * 5, (B, H, W, CH, CH, 3)),
        ("conv_ln", (B, H, W, CH, CH, 1), [P, P, P, P, P, 1, P, P, P, P], [P] * 8 + [None] + [P] * 5, (B, H, W, CH, CH, 1)),
    ]


# shapes the query refuses (it returns 0) and the call refuses with DCPT_ERR_ARG: (op, query arguments, arguments after ws_bytes)
_REFUSED_SHAPES = [
    ("conv3x3_act", (B, H, W, 6, CH), (B, H, W, 6, CH, 0.2)),
    ("up2_conv3x3_act", (B, H, W, 6), (B, H, W, 6, 0.2)),
    ("conv3x3_ps_out", (B, H, W, CH, 5, 3), (B, H, W, CH, 5, 3)),
    ("conv3x3_ps_out", (B, H, W, CH, 3, 5), (B, H, W, CH, 3, 5)),
    ("conv3conv_res", (B, H, W, 24), (B, H, W, 24)),
    ("rcab", (B, H, W, CH, 0), (B, H, W, CH, 0, 1.0)),
    ("conv3x3_ps", (B, H, W, CH, 4), (B, H, W, CH, 4)),
]


def _call(lib, name, direction, head, ws, ws_bytes, tail):
    tail = tuple(tail) + ((1,) if (name, direction) == ("conv_ln", "bwd") else ())   # conv_ln_bwd ends with the relu flag
    return getattr(lib, f"dcpt_{name}_{direction}")(*head, ws, ws_bytes, *tail, None)


def test_short_or_null_workspace_and_null_operand_are_refused(lib):
    for name, q, fwd_head, bwd_head, tail in _ops():
        for backward, direction, head in ((0, "fwd", fwd_head), (1, "bwd", bwd_head)):
            who = f"{name}_{direction}"
            need = getattr(lib, f"dcpt_{name}_ws_bytes")(*q, backward)
            assert need > 0, who
            for ws, ws_bytes in ((P, need - 1), (None, need)):
                assert _call(lib, name, direction, head, ws, ws_bytes, tail) == ERR_WS, who
                msg = lib.dcpt_last_error().decode()
                assert "workspace too small" in msg and who in msg, msg
            assert _call(lib, name, direction, [None] + head[1:], P, need, tail) == ERR_ARG, who


def test_shapes_the_query_refuses_are_refused_by_the_call(lib):
    heads = {name: (f, b) for name, _, f, b, _ in _ops()}
    for name, q, tail in _REFUSED_SHAPES:
        for backward, direction in ((0, "fwd"), (1, "bwd")):
            assert getattr(lib, f"dcpt_{name}_ws_bytes")(*q, backward) == 0, (name, q)
            assert _call(lib, name, direction, heads[name][backward], P, 1 << 16, tail) == ERR_ARG, (name, direction, q)
            assert name in lib.dcpt_last_error().decode()
