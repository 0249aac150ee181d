"""CPU: the yardstick of the resize kernel (tests/interp_restatement.py against ``F.interpolate`` on float64 tensors) and the surface of the
second-order degradation chain that needs no device: torch's size rule, the refusals of dcpt_interp_fwd, the host half of the chain
(``draw_second_order_plan``), RealESRGANDataset, ``degrade_collate`` on its samples and the shipped option file.

Bound of the restatement check: torch's float64 kernels and the restatement compute the same taps and differ in summation order only, by
about 1e-14 at |v| < 2 (measured below: 4.9e-15 at most in the issue's sweep); after the cast to fp32 both are roundings of numbers that
close, so they are equal or neighbours: at most one ulp of a value below 2, 2^-23."""
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import interp_restatement as R
from dcpt_amd.keyed_init import keyed_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 5, 7, 37, 53)
SCALES = (0.15, 0.37, 0.5, 1.0, 1.23, 1.5)
SIZES = (1, 3, 8, 40, 53, 60)
CHAIN_OPT = dict(resize_prob=[0.2, 0.7, 0.1], resize_range=[0.15, 1.5], gaussian_noise_prob=0.5, noise_range=[1, 30],
                 poisson_scale_range=[0.05, 3], gray_noise_prob=0.4, jpeg_range=[30, 95], second_blur_prob=0.8,
                 resize_prob2=[0.3, 0.4, 0.3], resize_range2=[0.3, 1.2], noise_range2=[1, 25], poisson_scale_range2=[0.05, 2.5],
                 gray_noise_prob2=0.4, jpeg_range2=[30, 95])


def _torch64(x, mode, **kw):
    extra = {} if mode == "area" else {"align_corners": False}
    return F.interpolate(x.double(), mode=mode, **kw, **extra)


@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_against_torch_float64(mode):
    worst64, worst32, n = 0.0, 0.0, 0
    for h in LENGTHS:
        for w in LENGTHS:
            x = keyed_input(f"interpcpu.{h}.{w}", (2, 2, h, w), lo=-0.5, hi=1.5)
            forms = [dict(scale_factor=s) for s in SCALES if math.floor(h * s) >= 1 and math.floor(w * s) >= 1]
            forms += [dict(scale_factor=(1.23, 0.37))] if math.floor(w * 0.37) >= 1 else []
            forms += [dict(size=(a, b)) for a, b in zip(SIZES, reversed(SIZES))]
            for kw in forms:
                want = _torch64(x, mode, **kw)
                got = R.interp_f64(x.numpy(), mode, **kw)
                assert got.shape == tuple(want.shape), (kw, got.shape, tuple(want.shape))
                worst64 = max(worst64, float(np.abs(got - want.numpy()).max()))
                worst32 = max(worst32, float(np.abs(got.astype(np.float32) - want.float().numpy()).max()))
                n += got.size
    print(f"{mode}: {n} outputs, largest float64 difference {worst64:.3e}, after the cast to fp32 {worst32:.3e} (bound 2^-23 = {2.0 ** -23:.3e})")
    assert worst32 <= 2.0 ** -23
    assert worst64 < 1e-13


def test_output_size_and_ratio_rules():
    from dcpt_amd import functional as DF

    for h in (7, 37, 67, 256):
        for sf in (0.15, 0.37, 0.5, 1.0, 1.23, 1.5, 0.2999, 1 / 3):
            (ho, wo), (rh, rw) = DF.interp_geometry((h, 2 * h + 1), scale_factor=sf)
            assert (ho, wo) == (math.floor(h * sf), math.floor((2 * h + 1) * sf)) and rh == rw == 1.0 / sf
            assert tuple(F.interpolate(torch.zeros(1, 1, h, 2 * h + 1), scale_factor=sf, mode="bilinear").shape[2:]) == (ho, wo)
    assert DF.interp_geometry((64, 80), scale_factor=(0.5, 1.5)) == ((32, 120), (2.0, 1.0 / 1.5))
    assert DF.interp_geometry((64, 80), size=(24, 30)) == ((24, 30), (64 / 24, 80 / 30))
    assert DF.interp_geometry((64, 80), size=7) == ((7, 7), (64 / 7, 80 / 7))
    assert DF.interp_geometry((67, 131), scale_factor=0.37)[0] == DF.interp_geometry((67, 131), size=(24, 48))[0]
    assert DF.interp_geometry((67, 131), scale_factor=0.37)[1] != DF.interp_geometry((67, 131), size=(24, 48))[1]
    for bad in (dict(), dict(size=4, scale_factor=2.0), dict(scale_factor=0.0), dict(scale_factor=-1.0), dict(scale_factor=(1.0, 2.0, 3.0)),
                dict(size=(0, 4)), dict(size=2.5), dict(scale_factor=0.01), dict(scale_factor=float("nan"))):
        with pytest.raises(ValueError):
            DF.interp_geometry((8, 8), **bad)


def test_entry_point_refusals_need_no_device():
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    ok = dict(x=1 << 20, y=1 << 24, B=2, C=3, H=8, W=8, Ho=4, Wo=4, mode=1, rh=2.0, rw=2.0, flags=0)

    def call(**over):
        a = {**ok, **over}
        return lib.dcpt_interp_fwd(a["x"], a["y"], a["B"], a["C"], a["H"], a["W"], a["Ho"], a["Wo"], a["mode"], a["rh"], a["rw"], a["flags"], None)

    for over, text in [(dict(x=None), b"null"), (dict(y=None), b"null"), (dict(mode=3), b"unknown mode"), (dict(mode=-1), b"unknown mode"),
                       (dict(flags=4), b"unknown flags"), (dict(Ho=0), b"bad shape"), (dict(B=0), b"bad shape"), (dict(W=-3), b"bad shape"),
                       (dict(H=1 << 16, W=(1 << 14) + 1), b"2^30"), (dict(Ho=(1 << 15) + 1, Wo=1 << 15), b"2^30"),
                       (dict(rh=0.0), b"ratios"), (dict(rw=float("nan")), b"ratios"), (dict(mode=2, rh=float("inf")), b"ratios"),
                       (dict(y=(1 << 20) + 64), b"overlaps")]:
        assert call(**over) != 0 and text in lib.dcpt_last_error(), (over, lib.dcpt_last_error())
    with pytest.raises(_lib.DcptHipError):
        DF.interpolate(torch.zeros(1, 1, 4, 4), scale_factor=2.0)
    with pytest.raises(_lib.DcptHipError):
        DF.interpolate(np.zeros((1, 1, 4, 4), dtype=np.float32), scale_factor=2.0)


# ---- the plan -----------------------------------------------------------------------------------------------
def _rng(seed):
    return random.Random(seed), np.random.RandomState(seed)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    return type(a) is type(b) and a == b


def _host_only(v):
    if isinstance(v, dict):
        return all(_host_only(x) for x in v.values())
    if torch.is_tensor(v):
        return v.device.type == "cpu"
    if isinstance(v, tuple):
        return all(isinstance(x, int) for x in v)
    return isinstance(v, (bool, int, float, str))


def test_plan_is_seeded_host_only_and_follows_the_size_formulas():
    from basicsr.data.degradations import RESIZE_MODES, draw_second_order_plan

    B, H, W = 3, 256, 200
    seen = {"final_first": set(), "second_blur": set(), "kind": set(), "mode": set()}
    for seed in range(40):
        for scale in (2, 4):
            plan = draw_second_order_plan(CHAIN_OPT, B, H, W, scale, rng=_rng(seed))
            assert _same(plan, draw_second_order_plan(CHAIN_OPT, B, H, W, scale, rng=_rng(seed)))
            assert _host_only(plan), plan
            s1, s2 = plan["resize1"]["scale_factor"], plan["resize2"]["scale_factor"]
            assert 0.15 <= s1 <= 1.5 and 0.3 <= s2 <= 1.2
            assert plan["resize2"]["size"] == (int(H / scale * s2), int(W / scale * s2))       # step 6
            assert plan["out_size"] == (H // scale, W // scale)                                  # step 8
            assert plan["resize1"]["mode"] in RESIZE_MODES and plan["resize2"]["mode"] in RESIZE_MODES and plan["final_mode"] in RESIZE_MODES
            for n, (lo, hi), (plo, phi) in ((plan["noise1"], (1, 30), (0.05, 3)), (plan["noise2"], (1, 25), (0.05, 2.5))):
                assert n["amp"].dtype == torch.float32 and n["gray"].dtype == torch.int32 and n["key"].dtype == torch.int64
                assert n["amp"].shape == n["gray"].shape == n["key"].shape == (B,)
                a, b = (lo, hi) if n["kind"] == "gaussian" else (plo, phi)
                assert bool(((n["amp"] >= a) & (n["amp"] <= b)).all()) and set(n["gray"].tolist()) <= {0, 1}
                assert n["key"].tolist() == [n["key"][0].item() + i for i in range(B)]
                seen["kind"].add(n["kind"])
            for q in (plan["jpeg1"], plan["jpeg2"]):
                assert q.dtype == torch.float32 and q.shape == (B,) and bool(((q >= 30) & (q <= 95)).all())
            seen["final_first"].add(plan["final_first"])
            seen["second_blur"].add(plan["second_blur"])
            seen["mode"].add(plan["final_mode"])
    assert seen == {"final_first": {True, False}, "second_blur": {True, False}, "kind": {"gaussian", "poisson"}, "mode": set(RESIZE_MODES)}
    # the process-wide generators serve when no pair is given
    random.seed(5)
    np.random.seed(5)
    a = draw_second_order_plan(CHAIN_OPT, B, H, W, 4)
    random.seed(5)
    np.random.seed(5)
    assert _same(a, draw_second_order_plan(CHAIN_OPT, B, H, W, 4))


def test_plan_directions_follow_resize_prob():
    from basicsr.data.degradations import draw_second_order_plan

    up = {**CHAIN_OPT, "resize_prob": [1, 0, 0], "resize_prob2": [0, 0, 1]}
    down = {**CHAIN_OPT, "resize_prob": [0, 1, 0], "resize_prob2": [0, 1, 0]}
    for seed in range(25):
        p = draw_second_order_plan(up, 2, 64, 64, 4, rng=_rng(seed))
        assert 1.0 <= p["resize1"]["scale_factor"] <= 1.5 and p["resize2"]["scale_factor"] == 1.0 and p["resize2"]["size"] == (16, 16)
        p = draw_second_order_plan(down, 2, 256, 256, 4, rng=_rng(seed))
        assert 0.15 <= p["resize1"]["scale_factor"] <= 1.0 and 0.3 <= p["resize2"]["scale_factor"] <= 1.0


def test_plan_refuses_sizes_below_the_reflect_padding():
    from basicsr.data.degradations import draw_second_order_plan

    draw_second_order_plan(CHAIN_OPT, 2, 256, 256, 4, rng=_rng(0))
    draw_second_order_plan(CHAIN_OPT, 2, 74, 74, 4, rng=_rng(0))                           # floor(74 * 0.15) = 11, 74 // 4 = 18
    with pytest.raises(ValueError, match="reflect padding"):
        draw_second_order_plan(CHAIN_OPT, 2, 73, 256, 4, rng=_rng(0))                      # floor(73 * 0.15) = 10
    with pytest.raises(ValueError, match="reflect padding"):
        draw_second_order_plan(CHAIN_OPT, 2, 256, 10, 1, rng=_rng(0))                      # the first blur itself
    with pytest.raises(ValueError, match="reflect padding"):
        draw_second_order_plan({**CHAIN_OPT, "resize_prob": [1, 0, 0]}, 2, 40, 40, 4, rng=_rng(0))   # lq of 10 x 10 under the sinc filter
    draw_second_order_plan({**CHAIN_OPT, "resize_prob": [1, 0, 0]}, 2, 44, 44, 4, rng=_rng(0))       # no downscale: 44 and 11 pass


# ---- the data set ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("realsr_gt")
    for i, (h, w) in enumerate([(40, 48), (33, 37), (48, 35)]):
        low = keyed_input(f"interpcpu.png{i}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0].clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / f"im{i}.png")
    return str(root)


def _set(kind, root, **over):
    from basicsr.data import build_dataset

    opt = dict(name=kind, type=kind, dataroot_gt=root, phase="train", gt_size=32, use_hflip=True, use_rot=False)
    opt.update(over)
    return build_dataset(opt)


def test_dataset_yields_three_kernels_and_no_lq(png_folder):
    ds = _set("RealESRGANDataset", png_folder, sinc_prob=0.5, sinc_prob2=0.5, blur_sigma2=[0.2, 1.5], final_sinc_prob=0.5)
    random.seed(11)
    np.random.seed(11)
    pulses = 0
    for i in range(12):
        s = ds[i % 3]
        assert sorted(s) == ["gt", "gt_path", "kernel1", "kernel2", "lq_path", "sinc_kernel"]
        assert tuple(s["gt"].shape) == (3, 32, 32)
        for k in ("kernel1", "kernel2", "sinc_kernel"):
            assert s[k].dtype == torch.float32 and tuple(s[k].shape) == (21, 21) and abs(float(s[k].double().sum()) - 1.0) < 1e-5, k
        pulse = torch.zeros(21, 21)
        pulse[10, 10] = 1.0
        pulses += int(torch.equal(s["sinc_kernel"], pulse))
    assert 0 < pulses < 12
    seeded = _set("RealESRGANDataset", png_folder, kernel_seed=3)
    again = _set("RealESRGANDataset", png_folder, kernel_seed=3)
    for i in range(3):
        a, b, c = seeded[i], seeded[i], again[i]
        for k in ("kernel1", "kernel2", "sinc_kernel"):
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k])
    assert not torch.equal(seeded[0]["kernel1"], seeded[1]["kernel1"])
    with pytest.raises(ValueError, match="final_sinc_prob"):
        _set("RealESRGANDataset", png_folder, final_sinc_prob=1.5)
    with pytest.raises(ValueError, match="gt_size"):
        _set("RealESRGANDataset", png_folder, gt_size=10)


def test_degrade_collate_takes_chain_batches_and_refuses_them_in_a_mixed_batch(png_folder):
    from torch.utils.data import default_collate

    from basicsr.data import degrade_collate

    chain = _set("RealESRGANDataset", png_folder, kernel_seed=1)
    blur = _set("PairedImageBlurDataset", png_folder, blur_backend="device")
    samples = [chain[i] for i in range(3)]
    got = degrade_collate([dict(s) for s in samples])
    assert list(got) == list(default_collate([dict(s) for s in samples])) and "degrade_kind" not in got and "lq" not in got
    assert tuple(got["kernel1"].shape) == tuple(got["kernel2"].shape) == tuple(got["sinc_kernel"].shape) == (3, 21, 21)
    with pytest.raises(ValueError, match="exactly one of"):
        degrade_collate([chain[0], blur[1]])


def test_the_shipped_option_file_parses_and_builds_the_dataset(png_folder):
    from basicsr.data.degradations import draw_second_order_plan
    from basicsr.utils.options import yaml_load

    opt = yaml_load(os.path.join(ROOT, "options", "realsr", "train_SwinIR_realSR_x4.yml"))
    assert opt["model_type"] == "SRModel" and opt["scale"] == 4
    assert opt["network_g"]["type"] == "SwinIR" and opt["network_g"]["upsampler"] == "nearest+conv" and opt["network_g"]["upscale"] == 4
    deg = opt["degradation"]
    for k, v in CHAIN_OPT.items():
        assert deg[k] == v, k
    train = dict(opt["datasets"]["train"])
    assert train["type"] == "RealESRGANDataset" and train["gt_size"] == 256
    assert train["kernel_prob"] == [0.45, 0.25, 0.12, 0.03, 0.12, 0.03] and train["blur_sigma2"] == [0.2, 1.5] and train["final_sinc_prob"] == 0.8
    train.update(dataroot_gt=png_folder, phase="train", gt_size=32)
    ds = _set(train.pop("type"), png_folder, **{k: v for k, v in train.items() if k not in ("name", "type")})
    assert sorted(ds[0]) == ["gt", "gt_path", "kernel1", "kernel2", "lq_path", "sinc_kernel"]
    plan = draw_second_order_plan(deg, 8, 256, 256, opt["scale"], rng=_rng(0))
    assert plan["out_size"] == (64, 64)
