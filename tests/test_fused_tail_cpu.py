"""CPU: the fused step tail (include/dcpt_hip.h dcpt_grad_norm / dcpt_adamw_step_ex, dcpt_amd.optim.FusedAdamW.step(max_grad_norm=, ema=),
``train.fused_step_tail``) as far as it goes without a device: the ABI additions, the workspace query, argument checks that return before
any launch, and which route SRModel / DCDistModel take (reference sr_model.py:166-174: clip_grad_norm_, optimizer.step(), model_ema())."""
import ctypes as C
import logging
import os
import re

import pytest
import torch

from kernel_trace import kernel_trace
from tests import test_plumbing_cpu as TP   # registers the CPU stand-in arch ``_TestConvArch``

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dcpt_grad_norm_ws_bytes", "dcpt_grad_norm", "dcpt_adamw_step_ex")


def test_header_and_ctypes_table_carry_the_three_names_and_the_abi_version():
    from dcpt_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcpt_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in dcpt_hip.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert "dcpt_adamw_step" in _lib.SIGNATURES   # the plain entry stays
    assert lib.dcpt_abi_version() == _lib.ABI_VERSION == 16


def test_grad_norm_workspace_query():
    from dcpt_amd import _lib

    lib = _lib.load()
    numel = (C.c_int64 * 4)(0, 1, 4096, 4097)
    assert lib.dcpt_grad_norm_ws_bytes(4, numel) == 8 * (0 + 1 + 1 + 2)
    assert lib.dcpt_grad_norm_ws_bytes(0, None) == 0
    assert lib.dcpt_grad_norm_ws_bytes(1, (C.c_int64 * 1)(2 ** 32 - 4097)) == 8 * (2 ** 32 // 4096 - 1)


def _hparams():
    from dcpt_amd.optim import _HParams

    return _HParams(1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 0.001, 0)


def test_bad_arguments_return_before_any_launch():
    from dcpt_amd import _lib

    lib = _lib.load()
    fake = (C.c_void_p * 1)(0x1000)   # never dereferenced: every call below returns from its argument checks
    one = (C.c_int64 * 1)(4097)
    h = _hparams()
    with kernel_trace() as t:
        # dcpt_grad_norm
        assert lib.dcpt_grad_norm(1, None, one, 1.0, 0x1000, 16, 0x1000, None) != 0 and b"null" in lib.dcpt_last_error()
        assert lib.dcpt_grad_norm(1, fake, one, 1.0, 0x1000, 16, None, None) != 0 and b"null" in lib.dcpt_last_error()
        assert lib.dcpt_grad_norm(1, (C.c_void_p * 1)(None), one, 1.0, 0x1000, 16, 0x1000, None) != 0 and b"null" in lib.dcpt_last_error()
        assert lib.dcpt_grad_norm(1, fake, one, 1.0, 0x1000, 8, 0x1000, None) != 0 and b"workspace" in lib.dcpt_last_error()
        assert lib.dcpt_grad_norm(1, fake, one, 1.0, None, 16, 0x1000, None) != 0 and b"workspace" in lib.dcpt_last_error()
        for bad in (-1, 2 ** 32 - 4096):
            assert lib.dcpt_grad_norm(1, fake, (C.c_int64 * 1)(bad), 1.0, 0x1000, 1 << 30, 0x1000, None) != 0
            assert b"elements" in lib.dcpt_last_error()
        # dcpt_adamw_step_ex
        assert lib.dcpt_adamw_step_ex(1, None, fake, fake, fake, None, one, C.byref(h), None, 0.0, None) != 0 and b"null" in lib.dcpt_last_error()
        assert lib.dcpt_adamw_step_ex(1, fake, fake, fake, fake, None, one, None, None, 0.0, None) != 0 and b"null" in lib.dcpt_last_error()
        assert lib.dcpt_adamw_step_ex(1, fake, fake, fake, fake, (C.c_void_p * 1)(None), one, C.byref(h), 0x1000, 0.9, None) != 0
        assert b"null pointer" in lib.dcpt_last_error()
        assert lib.dcpt_adamw_step_ex(1, fake, fake, fake, fake, fake, one, C.byref(h), None, 1.5, None) != 0 and b"ema_decay" in lib.dcpt_last_error()
        assert lib.dcpt_adamw_step_ex(1, fake, fake, fake, fake, None, (C.c_int64 * 1)(2 ** 32), C.byref(h), 0x1000, 0.0, None) != 0
        assert b"elements" in lib.dcpt_last_error()
    assert t.counts == {}, t.counts


# ---- models: which route a step takes ----------------------------------------------------------------------------------------------

def _train_opt(model_type="SRModel", **train):
    opt = TP._opt(model_type=model_type, is_train=True, grad_clip=0.01)
    opt["train"] = dict(pixel_opt=dict(type="L1Loss", loss_weight=1.0, reduction="mean"), optim_g=dict(type="Adam", lr=1e-3), ema_decay=0.9,
                        **train)
    return opt


class _Calls:
    """records clip_grad_norm_, optimizer_g.step(**kwargs) and model_ema() of one optimize_parameters"""

    def __init__(self, monkeypatch, model):
        self.log = []
        real_clip, real_step, real_ema = torch.nn.utils.clip_grad_norm_, model.optimizer_g.step, model.model_ema
        monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: (self.log.append("clip"), real_clip(*a, **k))[1])
        monkeypatch.setattr(model.optimizer_g, "step", lambda *a, **k: (self.log.append(("step", dict(k))), real_step(*a, **k))[1])
        monkeypatch.setattr(model, "model_ema", lambda *a, **k: (self.log.append("ema"), real_ema(*a, **k))[1])


def _feed(m):
    g = torch.Generator().manual_seed(5)
    m.feed_data({"lq": torch.rand(2, 3, 16, 16, generator=g), "gt": torch.rand(2, 3, 16, 16, generator=g)})


@pytest.mark.parametrize("key", [None, False, True])
def test_srmodel_keeps_the_default_route_without_the_key_or_without_the_library_optimizer(key, monkeypatch, caplog):
    from basicsr.models import build_model

    logging.getLogger("basicsr").propagate = True
    with caplog.at_level(logging.WARNING):
        m = build_model(_train_opt(**({} if key is None else {"fused_step_tail": key})))
    assert m.fused_step_tail is False
    warned = [r for r in caplog.records if "fused_step_tail" in r.getMessage()]
    assert len(warned) == (1 if key else 0)   # asked for, but optimizer_g is torch's Adam: one warning at set-up
    calls = _Calls(monkeypatch, m)
    _feed(m)
    m.optimize_parameters(1)
    assert calls.log == ["clip", ("step", {}), "ema"]


def test_srmodel_makes_the_one_call_when_the_key_is_on_and_the_optimizer_is_the_library_one(monkeypatch):
    from basicsr.models import build_model
    from dcpt_amd import functional as DF
    from dcpt_amd.optim import FusedAdamW

    class Stub(FusedAdamW):   # (the real one refuses CPU parameters: this test is about the call, not the numerics)
        def __init__(self):
            self.seen = []

        def zero_grad(self, set_to_none=True):
            pass

        def step(self, closure=None, **kw):
            self.seen.append(kw)

    m = build_model(_train_opt(fused_step_tail=True))
    m.optimizer_g = Stub()
    m._setup_fused_step_tail()
    assert m.fused_step_tail is True
    calls = _Calls(monkeypatch, m)
    inval = []
    monkeypatch.setattr(DF, "invalidate_packed_weights", lambda: inval.append(1))
    _feed(m)
    m.optimize_parameters(1)
    assert [c for c in calls.log if c in ("clip", "ema")] == [] and len(m.optimizer_g.seen) == 1 and inval == [1]
    kw = m.optimizer_g.seen[0]
    assert kw["max_grad_norm"] == 0.01 and kw["ema"][1] == 0.9
    src, dst = dict(m.net_g.named_parameters()), dict(m.net_g_ema.named_parameters())
    assert len(kw["ema"][0]) == len(dst) and all(kw["ema"][0][src[k]] is dst[k] for k in dst)
    # no clipping, no EMA configured: both arguments are None
    m.grad_clip, m.ema_decay = 0, 0
    m.optimize_parameters(2)
    assert m.optimizer_g.seen[1] == dict(max_grad_norm=None, ema=None)


def test_dcdist_model_reads_the_key_too(monkeypatch):
    """DCDistModel's own optimize_parameters: default route with torch's optimizer, and the set-up hook is the shared one"""
    from basicsr.models.degradation_classification_distillation_model import DCDistModel
    from basicsr.models.sr_model import SRModel

    assert DCDistModel._setup_fused_step_tail is SRModel._setup_fused_step_tail
    m = DCDistModel.__new__(DCDistModel)
    m.opt = dict(train=dict(fused_step_tail=True))
    m.optimizer_g = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(2))])
    m._setup_fused_step_tail()
    assert m.fused_step_tail is False
