"""GPU: the Gaussian-noise kernel of dcpt_amd/csrc/noise.hip (through dcpt_amd.functional.gaussian_noise, basicsr.data.degradations, the
``device`` backend of PairedImageDenoiseDataset, mixed batches of basicsr.data.degrade_collate and the models' ``feed_data``) against
tests/noise_restatement.py, the kernel-blind numpy restatement (Philox in integers, the transform in float64).

Bounds:
* plain, in place, noise_only, CLIP: ``|y - T| <= 2^-24 |T| + 1e-12`` with T the restatement's float64 value: the one fp32 rounding of the
  output (half an ulp is at most 2^-24 |T|) plus the slack of the fp64 log / sqrt / sincos (|n| < 6.8, sigma / 255 <= 0.2, |x| <= 1.1: a few
  1e-16 per element; below 2^-126 the fp32 spacing is 1.4e-45).  No element is excluded.
* ROUND8: every output lies on the 8-bit grid and equals the restatement's value rounded to fp32.  An element whose 255 T lies within
  1e-6 of a half-integer may land on the neighbouring grid value through a last-bit difference of the fp64 library; such elements are
  left out, at most 0.1 % of a case.  The keys of the cases were chosen so that the restatement leaves out NONE (asserted).
* everything else (sigma 0, batch independence, two runs, mixed batches, the model step) is bit for bit.

Every bounded case prints its figure before it asserts."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import noise_restatement as R
from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (shape, sigma per image, key per image, gray per image or None).  One element; one pixel of three channels (a partial quad); 105
# elements per image: the second image starts 4 bytes off a 16-byte boundary and both end in a partial quad, one gray (35 pixels per plane:
# planes 1 and 2 misaligned); one channel, whole quads; 1683 elements per image with sigma 0 / 15 / 50 and a gray image (561 pixels per
# plane: odd); 12480 elements = 3120 quads per image: more than one workgroup of 256 lanes in x, aligned throughout.
CASES = {
    "1x1x1x1": ((1, 1, 1, 1), [25.0], [11], None),
    "1x3x1x1": ((1, 3, 1, 1), [50.0], [12], [0]),
    "2x3x5x7": ((2, 3, 5, 7), [15.0, 25.0], [13, (1 << 63) - 1], [0, 1]),
    "3x1x6x6": ((3, 1, 6, 6), [5.0, 25.0, 50.0], [14, 15, -16], [1, 0, 0]),
    "3x3x17x33": ((3, 3, 17, 33), [0.0, 15.0, 50.0], [(3 << 32) | 17, 18, 0x0123456789ABCDEF], [0, 1, 0]),
    "2x3x64x65": ((2, 3, 64, 65), [25.0, 50.0], [20, 21], None),
}
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _args(name):
    shape, sigma, key, gray = CASES[name]
    x = keyed_input(f"gpunoise.{name}", shape, lo=-0.1, hi=1.1)   # (some samples beyond the clamp)
    return x, torch.tensor(sigma, dtype=torch.float32), torch.tensor(key, dtype=torch.int64), None if gray is None else torch.tensor(gray, dtype=torch.int32)


_REF = {}


def reference(name, **flags):
    """the restatement's float64 result for a case and flag set: computed once, shared, never modified"""
    k = (name, tuple(sorted(flags.items())))
    if k not in _REF:
        x, sigma, key, gray = _args(name)
        t = R.gauss_noise(x.numpy(), sigma.numpy(), key.tolist(), None if gray is None else gray.tolist(), **flags)
        t.setflags(write=False)
        _REF[k] = t
    return _REF[k]


def _within(y, t, what):
    d = np.abs(y.double().numpy() - t)
    bound = EPS32 * np.abs(t) + 1e-12
    worst = float((d / bound).max())
    print(f"{what}: max |y - T| {float(d.max()):.3e}; worst |y - T| / (2^-24 |T| + 1e-12) = {worst:.3f} over {d.size} elements")
    assert np.isfinite(y.numpy()).all() and worst <= 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_restatement(name, dev):
    """out of place, in place and noise_only, with host and with device parameters: one launch each"""
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    x, sigma, key, gray = _args(name)
    xd = x.to(dev)
    with kernel_trace() as t:
        y = DF.gaussian_noise(xd, sigma, key, gray)
        y2 = DF.gaussian_noise(xd, sigma.to(dev), key.to(dev), None if gray is None else gray.to(dev))
        z = xd.clone()
        zr = DF.gaussian_noise(z, sigma, key, gray, out=z)
        n = DF.gaussian_noise(xd, sigma, key, gray, noise_only=True)
    assert t.counts == {"noise.gauss": 4}, t.counts
    assert y.dtype == torch.float32 and y.shape == x.shape and y.is_contiguous() and y.data_ptr() != xd.data_ptr()
    assert torch.equal(_bits(xd.cpu()), _bits(x))                               # out of place: x untouched
    assert zr.data_ptr() == z.data_ptr()
    _within(y.cpu(), reference(name), f"gaussian_noise {name}")
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(z), _bits(y))   # device parameters and in place: the same bits
    _within(n.cpu(), reference(name, noise_only=True), f"gaussian_noise {name} noise_only")
    if gray is not None and x.shape[1] == 3:
        for b in range(x.shape[0]):
            same = bool(torch.equal(n[b, 0], n[b, 1]) and torch.equal(n[b, 0], n[b, 2]))
            assert same == bool(gray[b]) or float(sigma[b]) == 0.0, (b, same)


def test_sigma_zero_returns_x_bit_for_bit(dev):
    from dcpt_amd import functional as DF

    x, sigma, key, gray = _args("3x3x17x33")
    x[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, 1e-42, -3.5])
    y = DF.gaussian_noise(x.to(dev), sigma, key, gray).cpu()
    assert float(sigma[0]) == 0.0 and torch.equal(_bits(y[0]), _bits(x[0])) and not torch.equal(y[1], x[1])
    y = DF.gaussian_noise(x.to(dev), 0.0, 77, 1).cpu()
    assert torch.equal(_bits(y), _bits(x))
    assert bool((DF.gaussian_noise(x.to(dev), 0.0, 77, noise_only=True) == 0).all())


@pytest.mark.parametrize("name", ["2x3x5x7", "3x3x17x33", "2x3x64x65"])
def test_clip_and_round8(name, dev):
    from dcpt_amd import functional as DF

    x, sigma, key, gray = _args(name)
    xd = x.to(dev)
    y = DF.gaussian_noise(xd, sigma, key, gray, clip=True).cpu()
    _within(y, reference(name, clip=True), f"gaussian_noise {name} clip")
    assert float(y.min()) == 0.0 and float(y.max()) == 1.0 or name == "2x3x5x7"
    for clip in (False, True):
        y = DF.gaussian_noise(xd, sigma, key, gray, clip=clip, rounds=True).cpu()
        out = R.near_half(x.numpy(), sigma.numpy(), key.tolist(), None if gray is None else gray.tolist(), clip=clip)
        assert int(out.sum()) == 0, f"{name}: the restatement leaves out {int(out.sum())} elements near a half-integer; choose other keys"
        want = reference(name, clip=clip, rounds=True)
        v = y.double().numpy() * 255.0
        on_grid = np.abs(v - np.rint(v)) < 1e-4                     # (fp32 k / 255 times 255: within 255 * 2^-24 * 255 of the integer k)
        wrong = (y.numpy() != want.astype(np.float32)) & ~out
        print(f"gaussian_noise {name} rounds clip={clip}: {int(wrong.sum())} of {y.numel()} differ from the restatement, {int((~on_grid).sum())} "
              f"off the 8-bit grid, {int(out.sum())} left out (cap {y.numel() // 1000})")
        assert int(out.sum()) <= y.numel() // 1000 and bool(on_grid.all()) and int(wrong.sum()) == 0
        if clip:
            assert 0.0 <= float(y.min()) and float(y.max()) <= 1.0
        else:
            assert float(y.min()) < 0.0 and float(y.max()) > 1.0


def test_an_image_does_not_depend_on_its_batch(dev):
    """image b of a batch equals the same image run alone and at another batch position, bit for bit; two runs give the same bits"""
    from dcpt_amd import functional as DF

    for name in ("2x3x5x7", "3x3x17x33"):
        x, sigma, key, gray = _args(name)
        xd = x.to(dev)
        y = DF.gaussian_noise(xd, sigma, key, gray)
        assert torch.equal(_bits(DF.gaussian_noise(xd, sigma, key, gray)), _bits(y))
        B = x.shape[0]
        for b in range(B):
            alone = DF.gaussian_noise(xd[b:b + 1], sigma[b:b + 1], key[b:b + 1], gray[b:b + 1])
            assert torch.equal(_bits(alone[0]), _bits(y[b])), (name, b)
        perm = list(range(B))[::-1] + [0]                           # reversed, and image 0 once more at the end of a longer batch
        idx = torch.tensor(perm)
        moved = DF.gaussian_noise(xd[idx.to(dev)], sigma[idx], key[idx], gray[idx])
        for pos, b in enumerate(perm):
            assert torch.equal(_bits(moved[pos]), _bits(y[b])), (name, pos, b)


def test_outputs_stay_inside_their_buffers(dev):
    """the entry point on outputs of exactly the size they need, with a guard behind them, at the misaligned and ragged shapes; the outputs
    start as a NaN pattern, so an element the kernel skipped would show"""
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    with redzone() as rz:
        for name in ("1x3x1x1", "2x3x5x7", "3x3x17x33", "2x3x64x65"):
            x, sigma, key, gray = _args(name)
            B, C, H, W = x.shape
            for flags, ref in ((0, reference(name)), (4, reference(name, noise_only=True))):
                buf = DF._workspace(dev, 4 * x.numel())
                DF._call(lib.dcpt_gauss_noise_fwd, (None if flags else x.to(dev), sigma.to(dev), key.to(dev), None if gray is None else gray.to(dev), buf),
                         (B, C, H, W, flags), dev)
                _within(buf.view(torch.float32).reshape(x.shape).cpu(), ref, f"red zone {name} flags={flags}")
    assert rz.count == 8


def test_refusals_of_the_python_op(dev):
    from dcpt_amd import functional as DF

    x = keyed_input("gpunoise.bad", (2, 3, 8, 8)).to(dev)
    with pytest.raises(ValueError, match="negative"):
        DF.gaussian_noise(x, -1.0, 1)
    with pytest.raises(ValueError, match="negative"):
        DF.gaussian_noise(x, torch.tensor([5.0, -5.0]), 1)
    with pytest.raises(ValueError, match="sigma"):
        DF.gaussian_noise(x, torch.tensor([5.0, 5.0, 5.0]), 1)
    with pytest.raises(ValueError, match="key"):
        DF.gaussian_noise(x, 5.0, torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="64 bits"):
        DF.gaussian_noise(x, 5.0, 1 << 64)
    with pytest.raises(ValueError):
        DF.gaussian_noise(x[0], 5.0, 1)
    with pytest.raises(ValueError, match="out"):
        DF.gaussian_noise(x, 5.0, 1, out=torch.empty((2, 3, 8, 9), device=dev))
    with pytest.raises(NotImplementedError, match="inference-only"):
        DF.gaussian_noise(x.clone().requires_grad_(True), 5.0, 1)
    # a device sigma is not read back; a strided input is made contiguous; one key for every image gives every image the same noise
    y = DF.gaussian_noise(x.transpose(2, 3), torch.tensor([5.0, 5.0], device=dev), 9, noise_only=True)
    assert y.is_contiguous() and torch.equal(y[0], y[1]) and float(y.abs().max()) > 0


# ---- the reference's public functions ------------------------------------------------------------------
def test_the_pt_functions(dev):
    from kernel_trace import kernel_trace

    from basicsr.data import degradations as G

    img = keyed_input("gpunoise.pt", (3, 3, 9, 11)).to(dev)
    gray = torch.tensor([0.0, 1.0, 0.0])
    with kernel_trace() as t:
        noise = G.generate_gaussian_noise_pt(img, 20, gray, key=5)
        out = G.add_gaussian_noise_pt(img, 20, gray, clip=False, rounds=False, key=5)
    assert t.counts == {"noise.gauss": 2}, t.counts                 # one launch per call
    # out = fl(img + n) and img + noise = fl(img + fl(n)): the two exact sums differ by at most half an ulp of the noise, and rounding to
    # nearest is monotonic, so the two results are the same or neighbouring fp32 values: one ulp, taken at the largest of the magnitudes
    both = (img + noise).cpu()
    peak = torch.stack([out.cpu().abs(), both.abs(), noise.cpu().abs()]).amax(0).clamp_min(2.0 ** -126)
    ulp = torch.ldexp(torch.ones_like(peak), torch.frexp(peak).exponent - 24)
    d = (out.cpu() - both).abs()
    print(f"add_gaussian_noise_pt against img + generate_gaussian_noise_pt: worst {float((d / ulp).max()):.3f} ulp")
    assert bool((d <= ulp).all()) and float(noise.std()) * 255 > 10
    assert torch.equal(noise[1, 0], noise[1, 1]) and torch.equal(noise[1, 0], noise[1, 2]) and not torch.equal(noise[0, 0], noise[0, 1])
    assert not torch.equal(noise[0], noise[2])                      # image b uses key + b
    assert torch.equal(G.generate_gaussian_noise_pt(img[2:], 20, 0, key=7), noise[2:])
    # sigma as a per-image tensor, on the host or the device; a scalar gray_noise for every image
    per = G.generate_gaussian_noise_pt(img, torch.tensor([20.0, 20.0, 20.0], device=dev), gray.to(dev), key=5)
    assert torch.equal(per, noise)
    assert torch.equal(G.generate_gaussian_noise_pt(img, 20, 1, key=5)[1], noise[1])
    # clip and rounds as in the reference
    c = G.add_gaussian_noise_pt(img, 60, key=5)
    assert float(c.min()) == 0.0 and float(c.max()) == 1.0
    r = G.add_gaussian_noise_pt(img, 60, clip=True, rounds=True, key=5) * 255
    assert bool(((r - r.round()).abs() < 1e-4).all()) and 0 <= float(r.min()) and float(r.max()) <= 255
    # key=None: torch.manual_seed governs the noise, the random_* draws included
    for fn in (lambda: G.generate_gaussian_noise_pt(img, 20), lambda: G.add_gaussian_noise_pt(img, 20, gray),
               lambda: G.random_generate_gaussian_noise_pt(img, (5, 50), 0.5), lambda: G.random_add_gaussian_noise_pt(img, (5, 50), 0.5, clip=False)):
        torch.manual_seed(123)
        a = fn()
        b = fn()
        torch.manual_seed(123)
        a2 = fn()
        assert torch.equal(_bits(a), _bits(a2)) and not torch.equal(a, b) and a.shape == img.shape
    torch.manual_seed(4)
    n = G.random_generate_gaussian_noise_pt(img.expand(3, 3, 9, 11).repeat(8, 1, 1, 1), (10, 10), 0.5)
    grays = [bool(torch.equal(n[b, 0], n[b, 1])) for b in range(24)]
    std = float(n.std()) * 255
    print(f"random_generate_gaussian_noise_pt: {sum(grays)} of 24 images gray at gray_prob 0.5; noise std {std:.2f} at sigma 10")
    assert 0 < sum(grays) < 24 and 9.0 < std < 11.0


# ---- the data set, mixed batches and the models' feed_data ---------------------------------------------------
@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("noise_gt")
    for i, (h, w) in enumerate([(40, 48), (33, 37), (48, 35), (36, 36)]):
        low = keyed_input(f"gpunoise.png{i}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
        img = (img + keyed_input(f"gpunoise.png{i}.n", (3, h, w), lo=-0.05, hi=0.05)).clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / f"im{i}.png")
    return str(root)


def _set(kind, root, **over):
    from basicsr.data import build_dataset

    opt = dict(name=kind, type=kind, dataroot_gt=root, phase="train", gt_size=32, use_hflip=True, use_rot=True)
    opt.update(over)
    return build_dataset(opt)


def test_feed_data_on_a_noise_batch(png_folder, dev):
    """a single-kind ``noise_backend: device`` batch through the train loader: one launch, the restatement's noise, unclipped; a validation
    set shows the same noise on every visit"""
    from kernel_trace import kernel_trace

    from basicsr.data import build_dataloader
    from tests.test_gpu_jpeg import _sr_model

    model = _sr_model()
    ds = _set("PairedImageDenoiseDataset", png_folder, sigma_type="choice", sigma_range=[15, 50], noise_backend="device")
    random.seed(5)
    torch.manual_seed(5)
    batch = next(iter(build_dataloader(ds, dict(phase="train", batch_size_per_gpu=4, num_worker_per_gpu=0))))
    assert "lq" not in batch and "degrade_kind" not in batch and tuple(batch["noise_key"].shape) == (4,)
    with kernel_trace() as t:
        model.feed_data(batch)
    assert t.counts == {"noise.gauss": 1}, t.counts
    want = R.gauss_noise(batch["gt"].numpy(), batch["noise_sigma"].numpy(), batch["noise_key"].tolist())
    _within(model.lq.cpu(), want, "feed_data on a noise batch")
    assert torch.equal(model.gt.cpu(), batch["gt"]) and float(model.lq.min()) < 0.0   # not clipped, like the host path
    val = _set("PairedImageDenoiseDataset", png_folder, phase="val", sigma_range=25, noise_backend="device", noise_seed=3)
    seen = []
    for _ in range(2):
        model.feed_data(next(iter(build_dataloader(torch.utils.data.Subset(val, [1]), dict(phase="val")))))
        seen.append(model.lq.clone())
    assert torch.equal(_bits(seen[0]), _bits(seen[1])) and tuple(seen[0].shape) == (1, 3, 33, 37)


def _mixed_batch(root):
    """nine samples of six sets (the five kinds; demosaic with both methods), each drawn under a seed of its own so that the host-backend
    twin of a set sees the same crop, augmentation and strokes; returns the collated batch, the samples and their host twins"""
    from basicsr.data import degrade_collate

    D, J, M, I, P = "PairedImageDenoiseDataset", "PairedImageJPEGCARDataset", "PairedImageMosaicDataset", "PairedImageInpaintingDataset", "PairedImageDataset"
    sets = [(_set(D, root, sigma_type="choice", sigma_range=[15, 50], noise_backend="device"), None),
            (_set(J, root, q_type="choice", q_range=[10, 40], jpeg_backend="device"), None),
            (_set(M, root, demosaic_backend="device", demosaic_method="malvar"), _set(M, root, demosaic_method="malvar")),
            (_set(M, root, demosaic_backend="device", demosaic_method="bilinear"), _set(M, root, demosaic_method="bilinear")),
            (_set(I, root, inpaint_backend="device"), _set(I, root)),
            (_set(P, root), None)]
    order = [3, 0, 4, 5, 2, 1, 0, 3, 4]
    samples, twins = [], []
    for i, k in enumerate(order):
        random.seed(700 + i)
        samples.append(dict(sets[k][0][i % 4], dataset_idx=min(k, 4)))
        twin = None
        if sets[k][1] is not None:
            random.seed(700 + i)
            twin = sets[k][1][i % 4]
            assert torch.equal(twin["gt"], samples[-1]["gt"])
        twins.append(twin)
    return degrade_collate([dict(s) for s in samples]), samples, twins


def test_feed_data_on_a_mixed_batch(png_folder, dev):
    """per kind, the rows of ``lq`` are bit-identical to that kind's op on those gt rows alone; for demosaic and inpainting also to the host
    backends' ``lq``"""
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF
    from tests.test_gpu_jpeg import _sr_model

    batch, samples, twins = _mixed_batch(png_folder)
    kind = batch["degrade_kind"].tolist()
    assert kind == [3, 1, 4, 0, 3, 2, 1, 3, 4] and batch["mosaic"].tolist() == [1, 0, 1]
    model = _sr_model()
    with kernel_trace() as t:
        model.feed_data(batch)
    assert t.counts == {"noise.gauss": 1, "jpeg.fwd": 1, "degrade.demosaic": 2, "degrade.inpaint_lines": 1}, t.counts
    lq, gt = model.lq, batch["gt"].to(dev)
    assert lq.shape == gt.shape and torch.equal(model.gt, gt) and bool(torch.isfinite(lq).all())
    rows = {k: [i for i, v in enumerate(kind) if v == k] for k in range(5)}
    assert torch.equal(_bits(lq[rows[0]]), _bits(batch["lq"].to(dev)))
    assert torch.equal(_bits(lq[rows[1]]), _bits(DF.gaussian_noise(gt[rows[1]], batch["noise_sigma"], batch["noise_key"])))
    assert torch.equal(_bits(lq[rows[2]]), _bits(DF.diffjpeg(gt[rows[2]], batch["jpeg_quality"], uint8_io=True)))
    for i, m in zip(rows[3], batch["mosaic"].tolist()):
        assert torch.equal(_bits(lq[i:i + 1]), _bits(DF.demosaic(gt[i:i + 1], DF.DEMOSAIC_METHODS[m], uint8_io=True))), i
    assert torch.equal(_bits(lq[rows[4]]), _bits(DF.inpaint_lines(gt[rows[4]], batch["inpaint_lines"], batch["inpaint_meta"])))
    for i in rows[3] + rows[4]:
        assert torch.equal(_bits(lq[i].cpu()), _bits(twins[i]["lq"])), i       # the host backend's lq
    for i in range(len(kind)):
        assert kind[i] == 0 or not torch.equal(lq[i], gt[i]), i


def test_a_dcpt_step_on_a_mixed_batch_equals_the_step_on_the_explicit_lq(png_folder, dev):
    """one optimize_parameters of DCPTModel (tiny NAFNet + head) on the mixed batch against the same step fed that ``lq``: the same losses
    and parameter gradients, bit for bit"""
    from tests.test_gpu_jpeg import _dcpt_model

    batch, _, _ = _mixed_batch(png_folder)
    a = _dcpt_model()
    a.feed_data(batch)
    a.optimize_parameters(1)
    log_a = a.get_current_log()
    b = _dcpt_model()
    b.feed_data({"lq": a.lq.cpu(), "gt": batch["gt"], "dataset_idx": batch["dataset_idx"]})
    assert torch.equal(_bits(b.lq), _bits(a.lq))
    b.optimize_parameters(1)
    log_b = b.get_current_log()
    print(f"DCPTModel step on a mixed batch: {dict(log_a)} against {dict(log_b)}")
    assert list(log_a) == list(log_b) and "l_pix" in log_a and "l_classify" in log_a
    for k in log_a:
        assert log_a[k] == log_b[k], k
    moved = 0
    for na, nb in [(a.net_g, b.net_g), (a.net_dc, b.net_dc)]:
        for (k, p), r in zip(na.named_parameters(), nb.parameters()):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            assert torch.equal(_bits(p.grad), _bits(r.grad)), k
            moved += int(bool((p.grad != 0).any()))
    assert moved > 0


# ---- the command line on the shipped option file ---------------------------------------------------------
def test_train_cli_on_the_4d_device_options(png_folder):
    """``python basicsr/train.py -opt options/all_in_one/train/train_DCPT_NAFNet_4d_device.yml`` shortened through --force_yml to two
    iterations on a temporary PNG folder: four device-backend sets over one GT root -> ConcatDataset -> degrade_collate ->
    DCPTModel.feed_data -> the four kernels; the validation set takes the noise kernel"""
    yml = os.path.join(ROOT, "options", "all_in_one", "train", "train_DCPT_NAFNet_4d_device.yml")
    exp = os.path.join(ROOT, "experiments", "DCPT_NAFNet_4d_device")
    over = ["network_g:width=8", "network_g:enc_blk_nums=[1,1,1,1]", "network_dc:feature_dims=[8,16,32,64]", "datasets:train_1:batch_size_per_gpu=8",
            *[f"datasets:train_{k}:dataroot_gt={png_folder}" for k in (1, 2, 3, 4)], *[f"datasets:train_{k}:gt_size=32" for k in (1, 2, 3, 4)],
            f"datasets:val_1:dataroot_gt={png_folder}", "datasets:val_1:center_crop=32", "train:total_iter=2", "train:scheduler:periods=[2]",
            "logger:print_freq=1", "logger:save_checkpoint_freq=2", "val:val_freq=2"]
    shutil.rmtree(exp, ignore_errors=True)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "basicsr", "train.py"), "-opt", yml, "--force_yml", *over], cwd=ROOT,
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
        out = p.stdout + p.stderr
        assert p.returncode == 0, out[-3000:]
        for kind, name in (("PairedImageDenoiseDataset", "noise"), ("PairedImageJPEGCARDataset", "jpeg"), ("PairedImageMosaicDataset", "demosaic"),
                           ("PairedImageInpaintingDataset", "inpaint"), ("PairedImageDenoiseDataset", "val_noise25")):
            assert f"Dataset [{kind}] - {name} is built." in out, out[-3000:]
        for tag in ("l_pix", "l_classify"):
            losses = [float(v) for v in re.findall(tag + r": ([-0-9.eE+]+)", out)]
            assert len(losses) == 2 and all(0.0 < v < 20.0 for v in losses), out[-2000:]
        assert "# top1:" in out and os.path.exists(os.path.join(exp, "models", "net_dc_2.pth"))
    finally:
        shutil.rmtree(exp, ignore_errors=True)
