"""The bf16-storage entry points between and around the NAFBlock groups, of the classifier head, of Restormer and the NAFBlock itself refuse
a short or null workspace (DCPT_ERR_WS, "workspace too small" and the op's name in the message), a null first operand and a cached operand
image that is too small (DCPT_ERR_ARG, "packed weights too small") -- all before any launch, so no GPU is needed: a host buffer stands in
for device memory.  The bf16 twin of test_fp32_ops_refusal_cpu.py; tests/test_rcan_bf16_cpu.py covers the RCAN entry points."""
import ctypes as C

import pytest

ERR_ARG, ERR_WS = 1, 2
B, H, W, CH = 1, 8, 8, 16
M, N, K = 64, 16, 16   # the weight-gradient operator

_buf = (C.c_char * (1 << 20))()
P = C.addressof(_buf)


@pytest.fixture(scope="module")
def lib():
    from dcpt_amd import _lib

    return _lib.load()


def _struct(cls):
    return C.byref(cls(*([P] * len(cls._fields_))))


def _groups(wpacked_bytes=0):
    """the three conv -> LayerNorm groups of a bottleneck block; wpacked_bytes > 0: each with a cached operand image of that size"""
    from dcpt_amd._lib import BneckGroup

    g = (BneckGroup * 3)()
    for k in range(3):
        for name, _ in BneckGroup._fields_:
            setattr(g[k], name, P)
        g[k].wpacked = P if wpacked_bytes else None
        g[k].wpacked_bytes = wpacked_bytes
    return g


def _ops(wpacked_bytes=0):
    """(name in the messages, entry point, workspace query, query arguments, arguments in front of ws, arguments after ws_bytes).  The
    first argument is a required operand of every op.  wpacked_bytes > 0: the ops that take cached operand images only, with one of
    that size."""
    from dcpt_amd._lib import (GdfnParams, GdfnSaved, MdtaParams, MdtaSaved, NafBlockGrads, NafBlockParams, NafBlockSavedBf16)

    s = _struct
    pk = [P, wpacked_bytes] if wpacked_bytes else [None, 0]
    ops = []
    for k in (1, 3):
        t = (B, H, W, CH, CH, k)
        # conv_ln_fwd(x, w, wpacked, bytes, lnw, lnb, res, relu, z, y, mu, rstd, ...);  conv_ln_bwd(dy, x, w, wpacked, bytes, lnw, z, y, mu,
        # rstd, dx_add = NULL, dx, dw, dlnw, dlnb, dres, ..., relu)
        ops += [("conv_ln_fwd_bf16", "dcpt_conv_ln_fwd_bf16", "dcpt_conv_ln_bf16_ws_bytes", t + (0,), [P, P] + pk + [P, P, P, 1, P, P, P, P], t),
                ("conv_ln_bwd_bf16", "dcpt_conv_ln_bwd_bf16", "dcpt_conv_ln_bf16_ws_bytes", t + (1,),
                 [P, P, P] + pk + [P, P, P, P, P, None, P, P, P, P, P], t + (1,))]
    t = (B, H, W, CH, CH)
    ops += [("conv1x1_pool_relu_fwd_bf16", "dcpt_conv1x1_pool_relu_fwd_bf16", "dcpt_conv1x1_pool_relu_bf16_ws_bytes", t + (0,), [P, P] + pk + [P, P], t),
            ("conv1x1_pool_relu_bwd_bf16", "dcpt_conv1x1_pool_relu_bwd_bf16", "dcpt_conv1x1_pool_relu_bf16_ws_bytes", t + (1,),
             [P, P, P] + pk + [P, P, P], t)]
    t = (B, H, W, CH)
    ops += [("bottleneck_fwd_bf16", "dcpt_bottleneck_fwd_bf16", "dcpt_bottleneck_bf16_ws_bytes", t + (0,), [P, _groups(wpacked_bytes)], t),
            ("bottleneck_bwd_bf16", "dcpt_bottleneck_bwd_bf16", "dcpt_bottleneck_bf16_ws_bytes", t + (1,), [P, P, _groups(wpacked_bytes), P], t)]
    if wpacked_bytes:
        return ops
    ops += [("down2x2_fwd_bf16", "dcpt_down2x2_fwd_bf16", "dcpt_down2x2_bf16_ws_bytes", t + (0,), [P] * 4, t),
            ("down2x2_bwd_bf16", "dcpt_down2x2_bwd_bf16", "dcpt_down2x2_bf16_ws_bytes", t + (1,), [P] * 7, t),
            ("up_ps_fwd_bf16", "dcpt_up_ps_fwd_bf16", "dcpt_up_ps_bf16_ws_bytes", t + (0,), [P] * 4, t),
            ("up_ps_bwd_bf16", "dcpt_up_ps_bwd_bf16", "dcpt_up_ps_bf16_ws_bytes", t + (1,), [P] * 5, t)]
    for k in (1, 3):
        tk = (B, H, W, CH, CH, k)
        ops += [("conv_fwd_bf16", "dcpt_conv_fwd_bf16", "dcpt_conv_bf16_ws_bytes", tk + (0,), [P] * 3, tk),
                ("conv_bwd_bf16", "dcpt_conv_bwd_bf16", "dcpt_conv_bf16_ws_bytes", tk + (1,), [P] * 5, tk)]
    # the saved structs hold every optional tensor (full save mode): bit 1 of the queries' last argument
    tm, tg = (B, H, W, CH, 2), (B, H, W, CH, 32)   # 2 heads; hidden width 32
    ops += [("mdta_bf16_fwd", "dcpt_mdta_bf16_fwd", "dcpt_mdta_bf16_ws_bytes", tm + (2,), [s(MdtaParams), P, P, s(MdtaSaved)], tm + (0,)),
            ("mdta_bf16_bwd", "dcpt_mdta_bf16_bwd", "dcpt_mdta_bf16_ws_bytes", tm + (3,),
             [s(MdtaParams), s(MdtaParams), P, s(MdtaSaved), P, P], tm + (0,)),
            ("gdfn_bf16_fwd", "dcpt_gdfn_bf16_fwd", "dcpt_gdfn_bf16_ws_bytes", tg + (2,), [s(GdfnParams), P, P, s(GdfnSaved)], tg + (0,)),
            ("gdfn_bf16_bwd", "dcpt_gdfn_bf16_bwd", "dcpt_gdfn_bf16_ws_bytes", tg + (3,),
             [s(GdfnParams), s(GdfnParams), P, s(GdfnSaved), P, P], tg + (0,))]
    ops += [("nafblock_fwd_bf16", "dcpt_nafblock_fwd_bf16", "dcpt_nafblock_fwd_bf16_ws_bytes", t,
             [s(NafBlockParams), None, 0, P, P, s(NafBlockSavedBf16)], t),
            ("nafblock_bwd_bf16", "dcpt_nafblock_bwd_bf16", "dcpt_nafblock_bwd_bf16_ws_bytes", t,
             [s(NafBlockParams), None, 0, s(NafBlockGrads), P, s(NafBlockSavedBf16), P, P], t),
            ("conv1x1_wgrad_bf16", "dcpt_conv1x1_wgrad_bf16", "dcpt_conv1x1_wgrad_bf16_ws_bytes", (M, N, K), [P] * 4, (M, N, K))]
    return ops


def test_short_or_null_workspace_and_null_operand_are_refused(lib):
    for who, fn, query, q, head, tail in _ops():
        need = getattr(lib, query)(*q)
        assert 0 < need <= len(_buf), (who, need)
        call = getattr(lib, fn)
        for ws, ws_bytes in ((P, need - 1), (None, need)):
            assert call(*head, ws, ws_bytes, *tail, None) == ERR_WS, who
            msg = lib.dcpt_last_error().decode()
            assert "workspace too small" in msg and who in msg, msg
        assert call(None, *head[1:], P, need, *tail, None) == ERR_ARG, who


def test_short_cached_operand_images_are_refused(lib):
    for who, fn, query, q, head, tail in _ops(wpacked_bytes=16):
        need = getattr(lib, query)(*q)
        assert getattr(lib, fn)(*head, P, need, *tail, None) == ERR_ARG, who
        msg = lib.dcpt_last_error().decode()
        assert "packed weights too small" in msg and who in msg, msg
