"""CPU: RCAN is registered with the reference's state-dict layout (against the golden fixtures of the real reference at x2 / x3 / x4),
its guards hold, the new C-ABI entry points (dcpt_rcab_*, dcpt_conv3x3_ps_*) answer workspace queries and report bad arguments without
a GPU, there is no CPU fallback, and the training crop follows the reference's paired_random_crop at scale s."""
import os
import random

import numpy as np
import pytest
import torch

TINY = dict(num_in_ch=3, num_out_ch=3, num_feat=32, num_group=2, num_block=2)


def _build(**kw):
    import basicsr.archs  # noqa: F401  (registers the archs)
    from basicsr.utils.registry import ARCH_REGISTRY

    return ARCH_REGISTRY.get("RCAN")(**kw)


def test_rcan_is_registered():
    import basicsr.archs  # noqa: F401
    from basicsr.utils.registry import ARCH_REGISTRY

    assert "RCAN" in ARCH_REGISTRY


@pytest.mark.parametrize("s", [2, 3, 4])
def test_state_dict_matches_reference_tiny(golden_dir, s):
    g = np.load(os.path.join(golden_dir, f"rcan_tiny_x{s}.npz"))
    net = _build(upscale=s, **TINY)
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g["key_shapes"])
    net.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)


def test_state_dict_matches_reference_default(golden_dir):
    g = np.load(os.path.join(golden_dir, "rcan_full.npz"))
    net = _build(num_in_ch=3, num_out_ch=3)
    sd = net.state_dict()
    assert len(sd) == int(g["n_keys"]) == 1310
    assert list(sd.keys()) == list(g["keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g["key_shapes"])
    assert sum(p.numel() for p in net.parameters()) == int(g["n_params"])
    assert "mean" not in sd and tuple(net.mean.shape) == (1, 3, 1, 1)   # a plain attribute, as in the reference
    net.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)


def test_unsupported_options_raise():
    with pytest.raises(ValueError):
        _build(upscale=5, **TINY)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        _build(num_in_ch=3, num_out_ch=3, num_feat=30, num_group=1, num_block=1)


def test_no_cpu_fallback_for_rcan():
    from dcpt_amd import _lib

    net = _build(upscale=2, **TINY)
    with pytest.raises(_lib.DcptHipError):
        net(torch.zeros(1, 3, 8, 8))


def test_workspace_queries_need_no_gpu():
    from dcpt_amd import _lib

    lib = _lib.load()
    M = 16 * 48 * 48
    f, b = lib.dcpt_rcab_ws_bytes(16, 48, 48, 64, 4, 0), lib.dcpt_rcab_ws_bytes(16, 48, 48, 64, 4, 1)
    assert f >= 2 * M * 64 * 4 and b >= 2 * M * 64 * 4   # h / t (forward without saved), dt / dh (backward)
    pf, pb = lib.dcpt_conv3x3_ps_ws_bytes(16, 48, 48, 64, 2, 0), lib.dcpt_conv3x3_ps_ws_bytes(16, 48, 48, 64, 2, 1)
    assert pf >= 2 * 9 * 256 * 64 * 4 and pb >= M * 256 * 4
    assert lib.dcpt_conv3x3_ps_ws_bytes(1, 8, 8, 64, 3, 1) > lib.dcpt_conv3x3_ps_ws_bytes(1, 8, 8, 64, 2, 1)
    assert lib.dcpt_conv3x3_ps_ws_bytes(1, 8, 8, 64, 4, 0) == 0 and lib.dcpt_rcab_ws_bytes(1, 8, 8, 30, 2, 0) == 0


def test_bad_arguments_are_reported_not_crashed():
    from dcpt_amd import _lib

    lib = _lib.load()
    p, g = _lib.RcabParams(*([1] * 8)), _lib.RcabParams(*([1] * 8))
    sv = _lib.RcabSaved(*([1] * 4))
    assert lib.dcpt_rcab_fwd(None, 1, 1, None, None, 0, 2, 8, 8, 64, 4, 1.0, None) != 0 and b"null" in lib.dcpt_last_error()
    assert lib.dcpt_rcab_fwd(p, None, 1, None, None, 0, 2, 8, 8, 64, 4, 1.0, None) != 0 and b"null" in lib.dcpt_last_error()
    assert lib.dcpt_rcab_fwd(p, 1, 1, _lib.RcabSaved(1, 1, None, 1), None, 0, 2, 8, 8, 64, 4, 1.0, None) != 0 and b"saved" in lib.dcpt_last_error()
    assert lib.dcpt_rcab_fwd(p, 1, 1, None, None, 0, 2, 8, 8, 30, 2, 1.0, None) != 0 and b"multiple of 4" in lib.dcpt_last_error()
    assert lib.dcpt_rcab_fwd(p, 1, 1, None, None, 0, 2, 8, 8, 64, 0, 1.0, None) != 0 and b"Cr" in lib.dcpt_last_error()
    assert lib.dcpt_rcab_fwd(p, 1, 1, None, None, 0, 2, 8, 8, 64, 4, 1.0, None) != 0 and b"workspace" in lib.dcpt_last_error()
    assert lib.dcpt_rcab_bwd(p, g, 1, None, 1, 1, None, 0, 2, 8, 8, 64, 4, 1.0, None) != 0 and b"null" in lib.dcpt_last_error()
    assert lib.dcpt_rcab_bwd(p, g, 1, sv, 1, 1, None, 0, 2, 8, 8, 64, 4, 1.0, None) != 0 and b"workspace" in lib.dcpt_last_error()
    assert lib.dcpt_conv3x3_ps_fwd(1, 1, None, 1, None, 0, 1, 8, 8, 64, 2, None) != 0 and b"null" in lib.dcpt_last_error()
    assert lib.dcpt_conv3x3_ps_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 30, 2, None) != 0 and b"multiple of 4" in lib.dcpt_last_error()
    for r in (1, 4):
        assert lib.dcpt_conv3x3_ps_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 64, r, None) != 0 and b"r 2 or 3" in lib.dcpt_last_error()
        assert lib.dcpt_conv3x3_ps_bwd(1, 1, 1, 1, 1, 1, None, 0, 1, 8, 8, 64, r, None) != 0 and b"r 2 or 3" in lib.dcpt_last_error()
    assert lib.dcpt_conv3x3_ps_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 64, 3, None) != 0 and b"workspace" in lib.dcpt_last_error()
    assert lib.dcpt_conv3x3_ps_bwd(1, 1, 1, None, 1, 1, None, 0, 1, 8, 8, 64, 2, None) != 0 and b"null" in lib.dcpt_last_error()


# ---- the scale-aware training crop ----------------------------------------------------------------------------------------------------
def _pair(scale, h, w):
    lq = torch.arange(3 * h * w, dtype=torch.float32).reshape(3, h, w)
    gt = lq.repeat_interleave(scale, 1).repeat_interleave(scale, 2)   # GT pixel (y, x) carries LQ pixel (y // s, x // s)
    return lq, gt


def test_crop_at_scale_4_is_co_located():
    from basicsr.data import paired_random_crop_augment

    lq, gt = _pair(4, 30, 40)
    random.seed(5)
    for _ in range(20):
        a, b = paired_random_crop_augment(lq, gt, dict(gt_size=48, scale=4))
        assert tuple(a.shape) == (3, 12, 12) and tuple(b.shape) == (3, 48, 48)
        assert torch.equal(b, a.repeat_interleave(4, 1).repeat_interleave(4, 2))
    random.seed(6)
    a, b = paired_random_crop_augment(lq, gt, dict(gt_size=48, scale=4, use_hflip=True, use_rot=True))
    assert torch.equal(b, a.repeat_interleave(4, 1).repeat_interleave(4, 2))
    with pytest.raises(ValueError):
        paired_random_crop_augment(lq, gt[:, :-1], dict(gt_size=48, scale=4))


def test_crop_at_scale_1_keeps_its_draws():
    """scale 1 (or no scale): top = randint(0, h - size), left = randint(0, w - size), then one random() per flip / rotation in the
    order hflip, vflip, rot90 -- the same draws and slices of both images"""
    from basicsr.data import paired_random_crop_augment

    lq = torch.rand(3, 21, 34)
    gt = torch.rand(3, 21, 34)
    opt = dict(gt_size=16, use_hflip=True, use_rot=True)
    for seed in range(6):
        for o in (opt, dict(opt, scale=1)):
            random.seed(seed)
            a, b = paired_random_crop_augment(lq, gt, o)
            after = random.random()
            random.seed(seed)
            top, left = random.randint(0, 21 - 16), random.randint(0, 34 - 16)
            hflip, vflip, rot = random.random() < 0.5, random.random() < 0.5, random.random() < 0.5
            want = []
            for t in (lq, gt):
                t = t[:, top:top + 16, left:left + 16]
                if hflip:
                    t = t.flip(2)
                if vflip:
                    t = t.flip(1)
                if rot:
                    t = t.transpose(1, 2)
                want.append(t)
            assert torch.equal(a, want[0]) and torch.equal(b, want[1])
            assert after == random.random()   # no other draws
