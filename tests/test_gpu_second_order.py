"""GPU: the second-order degradation chain of basicsr/data/degradations.py (``draw_second_order_plan`` / ``apply_second_order``) and its
way through RealESRGANDataset, ``degrade_collate`` and ``SRModel.feed_data``.

The chain is a composition of device ops that have their own tests, so the checks here are of the composition: with a fixed plan the chain
equals the ops called one by one in this file (``torch.equal``: every op gives the same bits on every run); and up to the first resize it
is compared with the host forms (``filter2d_host``, bit for bit the blur kernel's result, then tests/interp_restatement.py) within 2^-23,
the bound of tests/test_gpu_interp.py: blurred values of a [0, 1] image under a normalised non-negative kernel stay in [0, 1], so |v| < 2.

Shapes: 2 x 3 x 64 x 80 at x4 and x2.  Plan A (x4): first resize by 0.73 to 46 x 58 -- no multiple of 16, so the JPEG pads macroblocks on
both edges --, the second blur, the final resize before the last JPEG.  Plan B (x2): "keep" in the first resize, no second blur, the last
JPEG before the final resize."""
import random

import numpy as np
import pytest
import torch

import interp_restatement as R
from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 80
OPT = dict(resize_prob=[0.2, 0.7, 0.1], resize_range=[0.5, 1.5], gaussian_noise_prob=0.5, noise_range=[1, 30], poisson_scale_range=[0.05, 3],
           gray_noise_prob=0.4, jpeg_range=[30, 95], second_blur_prob=0.8, resize_prob2=[0.3, 0.4, 0.3], resize_range2=[0.3, 1.2],
           noise_range2=[1, 25], poisson_scale_range2=[0.05, 2.5], gray_noise_prob2=0.4, jpeg_range2=[30, 95])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _noise(kind, amp, gray, key):
    return {"kind": kind, "amp": torch.tensor(amp, dtype=torch.float32), "gray": torch.tensor(gray, dtype=torch.int32),
            "key": torch.tensor([key, key + 1], dtype=torch.int64)}


def _plan(tag):
    from basicsr.data.degradations import draw_second_order_plan

    scale = 4 if tag == "A" else 2
    plan = draw_second_order_plan(OPT, B, H, W, scale, rng=(random.Random(7), np.random.RandomState(7)))   # the keys and sizes of a real plan
    assert plan["out_size"] == (H // scale, W // scale)
    if tag == "A":
        plan.update(resize1={"scale_factor": 0.73, "mode": "bicubic"}, noise1=_noise("gaussian", [12.0, 25.0], [0, 1], 1234),
                    second_blur=True, resize2={"scale_factor": 0.9, "size": (int(H / 4 * 0.9), int(W / 4 * 0.9)), "mode": "area"},
                    noise2=_noise("poisson", [0.5, 2.0], [1, 0], 99), final_first=True, final_mode="bilinear")
    else:
        plan.update(resize1={"scale_factor": 1.0, "mode": "area"}, noise1=_noise("poisson", [1.5, 0.3], [0, 0], 77),
                    second_blur=False, resize2={"scale_factor": 1.2, "size": (int(H / 2 * 1.2), int(W / 2 * 1.2)), "mode": "bilinear"},
                    noise2=_noise("gaussian", [20.0, 3.0], [1, 1], 5), final_first=False, final_mode="bicubic")
    plan["jpeg1"] = torch.tensor([35.0, 90.0])
    plan["jpeg2"] = torch.tensor([60.5, 42.0])
    return plan


def _inputs():
    gt = keyed_input("gpuchain.gt", (B, 3, H // 4, W // 4))
    gt = torch.nn.functional.interpolate(gt, size=(H, W), mode="bilinear", align_corners=False).clamp(0, 1)   # (smooth, so the JPEG keeps it)
    kernels = []
    for name in ("k1", "k2", "sinc"):
        k = keyed_input(f"gpuchain.{name}", (B, 21, 21)) ** 4
        kernels.append(k / k.sum(dim=(1, 2), keepdim=True))
    return (gt, *kernels)


def _one_by_one(gt, k1, k2, sinc, plan):
    """the steps of the issue, written out on the public ops"""
    from dcpt_amd import functional as DF

    def noise(out, n):
        if n["kind"] == "gaussian":
            return DF.gaussian_noise(out, n["amp"], n["key"], gray=n["gray"], clip=True)
        return DF.poisson_noise(out, n["amp"], n["key"], gray=n["gray"], clip=True)

    def final(out):
        return DF.filter2d(DF.interpolate(out, size=plan["out_size"], mode=plan["final_mode"]), sinc)

    out = DF.filter2d(gt, k1)
    out = DF.interpolate(out, scale_factor=plan["resize1"]["scale_factor"], mode=plan["resize1"]["mode"])
    out = noise(out, plan["noise1"])
    out = DF.diffjpeg(torch.clamp(out, 0, 1), plan["jpeg1"], differentiable=False, uint8_io=False)
    if plan["second_blur"]:
        out = DF.filter2d(out, k2)
    out = DF.interpolate(out, size=plan["resize2"]["size"], mode=plan["resize2"]["mode"])
    out = noise(out, plan["noise2"])
    if plan["final_first"]:
        out = DF.diffjpeg(torch.clamp(final(out), 0, 1), plan["jpeg2"], differentiable=False, uint8_io=False)
    else:
        out = final(DF.diffjpeg(torch.clamp(out, 0, 1), plan["jpeg2"], differentiable=False, uint8_io=False))
    return torch.round(torch.clamp(out, 0, 1) * 255) / 255


@pytest.mark.parametrize("tag", ["A", "B"])
def test_chain_equals_the_ops_one_by_one(tag, dev):
    from kernel_trace import kernel_trace

    from basicsr.data.degradations import apply_second_order, second_order_steps

    gt, k1, k2, sinc = _inputs()
    gtd, plan = gt.to(dev), _plan(tag)
    scale = plan["scale"]
    with kernel_trace() as t:
        lq = apply_second_order(gtd, k1, k2, sinc, plan)
    blurs = 3 if plan["second_blur"] else 2
    assert t.counts["degrade.interp"] == 3 and t.counts["degrade.filter2d"] == blurs and t.counts["jpeg.fwd"] == 2, t.counts
    assert t["noise.gauss"] == 1 and t["noise.poisson"] == 1, t.counts
    assert lq.dtype == torch.float32 and tuple(lq.shape) == (B, 3, H // scale, W // scale)
    assert float(lq.min()) >= 0.0 and float(lq.max()) <= 1.0 and torch.equal(lq, torch.round(lq * 255) / 255)   # the 8-bit grid
    assert torch.equal(gtd.cpu(), gt)                                                                          # gt untouched
    want = _one_by_one(gtd, k1.to(dev), k2.to(dev), sinc.to(dev), plan)
    assert torch.equal(lq, want)
    assert torch.equal(lq, apply_second_order(gtd, k1, k2, sinc, plan))                                       # a plan is a value: the same lq again
    assert float((lq - torch.nn.functional.interpolate(gtd, size=lq.shape[2:], mode="area")).abs().mean()) > 1e-3   # it did degrade
    steps = dict(second_order_steps(gtd, k1, k2, sinc, plan))
    names = list(steps)
    assert names[:4] == ["blur1", "resize1", "noise1", "jpeg1"] and ("blur2" in names) == plan["second_blur"]
    assert names[-3:] == (["final", "jpeg2", "lq"] if plan["final_first"] else ["jpeg2", "final", "lq"])
    s1 = plan["resize1"]["scale_factor"]
    assert tuple(steps["jpeg1"].shape[2:]) == (int(H * s1), int(W * s1)) and tuple(steps["noise2"].shape[2:]) == plan["resize2"]["size"]
    if tag == "A":
        assert tuple(steps["jpeg1"].shape[2:]) == (46, 58)                                                     # no multiple of 16


def test_chain_up_to_the_first_resize_against_the_host_forms(dev):
    from basicsr.data import filter2d_host
    from basicsr.data.degradations import second_order_steps

    gt, k1, k2, sinc = _inputs()
    for tag in ("A", "B"):
        plan = _plan(tag)
        plan["noise1"] = _noise("gaussian", [0.0, 0.0], [0, 0], 1)
        plan["noise2"] = _noise("gaussian", [0.0, 0.0], [0, 0], 2)
        steps = dict(second_order_steps(gt.to(dev), k1, k2, sinc, plan))
        blurred = torch.stack([filter2d_host(gt[b], k1[b]) for b in range(B)])
        assert torch.equal(steps["blur1"].cpu(), blurred)
        want = R.interp_f32(blurred.numpy(), plan["resize1"]["mode"], scale_factor=plan["resize1"]["scale_factor"])
        d = float((steps["resize1"].cpu().double() - torch.from_numpy(want).double()).abs().max())
        print(f"plan {tag}: blur + {plan['resize1']['mode']} resize by {plan['resize1']['scale_factor']} against the host forms: max |d| {d:.3e}")
        assert d <= 2.0 ** -23
        assert torch.equal(steps["noise1"], steps["resize1"].clamp(0, 1))                                      # sigma 0: only the clip


@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("chain_gt")
    for i, (h, w) in enumerate([(70, 90), (64, 64), (80, 66)]):
        low = keyed_input(f"gpuchain.png{i}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0].clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / f"im{i}.png")
    return str(root)


def _model(degradation):
    from basicsr.models import build_model
    from tests.test_gpu_jpeg import SWIN_TINY

    opt = dict(name="t", model_type="SRModel", scale=4, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True, degradation=degradation,
               network_g=dict(type="SwinIR", **{**SWIN_TINY, "upscale": 4, "upsampler": "nearest+conv"}), path=dict(pretrain_network_g=None),
               train=dict(pixel_opt=dict(type="L1Loss"), optim_g=dict(type="SGD", lr=0.05)))
    return build_model(opt)


def test_feed_data_on_a_batch_of_the_dataset(png_folder, dev):
    from kernel_trace import kernel_trace

    from basicsr.data import build_dataset, degrade_collate
    from basicsr.utils import USMSharp

    ds = build_dataset(dict(name="chain", type="RealESRGANDataset", dataroot_gt=png_folder, phase="train", gt_size=64, use_hflip=True,
                            use_rot=False, sinc_prob=0.1, sinc_prob2=0.1, blur_sigma2=[0.2, 1.5], kernel_seed=4))
    random.seed(21)
    np.random.seed(21)
    batch = degrade_collate([ds[i] for i in range(3)])
    assert "lq" not in batch and tuple(batch["kernel1"].shape) == (3, 21, 21)
    plain = _model(dict(OPT))
    with kernel_trace() as t:
        plain.feed_data(batch)
    assert t["degrade.interp"] == 3 and t["jpeg.fwd"] == 2 and t["degrade.filter2d"] in (2, 3), t.counts
    assert tuple(plain.lq.shape) == (3, 3, 16, 16) and plain.lq.is_cuda and torch.equal(plain.lq, torch.round(plain.lq * 255) / 255)
    assert torch.equal(plain.gt.cpu(), batch["gt"])
    sharp = _model(dict(OPT, gt_usm=True))
    sharp.feed_data(batch)
    assert tuple(sharp.lq.shape) == (3, 3, 16, 16) and tuple(sharp.gt.shape) == (3, 3, 64, 64)
    assert torch.equal(sharp.gt, USMSharp().to(dev)(batch["gt"].to(dev))) and not torch.equal(sharp.gt.cpu(), batch["gt"])
    with pytest.raises(ValueError, match="degradation"):
        _model(None).feed_data(batch)
    output = plain.net_g(plain.lq)
    assert tuple(output.shape) == tuple(plain.gt.shape)
