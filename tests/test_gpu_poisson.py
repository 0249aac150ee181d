"""GPU: the Poisson-noise kernels of dcpt_amd/csrc/noise.hip (through dcpt_amd.functional.poisson_noise, basicsr.data.degradations, the
``noise_type: poisson`` samples of PairedImageDenoiseDataset and the models' ``feed_data``) against tests/poisson_restatement.py, the
kernel-blind numpy restatement (levels and their count, Philox in integers, the upward search in float64).  The cases and what each
exercises: tests/poisson_cases.py.

Bounds:
* ``vals`` equals the restatement's exactly, and so does the count k of EVERY element, recovered from the fp32 noise_only output at scale 1
  as ``rint((t + l / 255) vals)``: t = k / vals - l / 255 is at most 256 / vals in magnitude, so its fp32 rounding moves (t + l / 255) vals
  by at most 256 * 2^-24, far from the 0.5 that would change the rint.
* plain, in place, noise_only, CLIP: ``|y - T| <= 2^-24 |T| + 1e-12`` with T the restatement's float64 value, the bound of the Gaussian
  tests: the one fp32 rounding of the output.  Given the same k the fp64 arithmetic behind T is a handful of correctly rounded operations,
  the same on both sides.
* Two kinds of element could differ for a reason that is not a fault, and the restatement reports both: (a) 255 v within 1e-9 of a
  half-integer (a level, and with it U, could flip); (b) a partial sum S_{k-1} or S_k within 2^-40 of u (k could flip).  (b): both sides
  run the same correctly rounded recurrence from p = exp(-lambda), so their sums differ only by the one- or two-ulp difference of the two
  ``exp`` implementations carried through s (relative 2^-52, s <= 1) -- the search's own rounding, at most about k 2^-53 <= 5e-14, is the
  same on both sides.  2^-40 = 9e-13 covers that ten times over, and the chance of an element inside it is about 4e-12.  Cap: 0.1 % of a
  case; the keys and inputs of every case are chosen so that the restatement excludes NONE, which is asserted (here and on the CPU in
  tests/test_poisson_cpu.py).
* ROUND8: every output lies on the 8-bit grid and equals the restatement's value rounded to fp32; an element whose 255 T lies within 1e-6
  of a half-integer is left out, at most 0.1 % of a case, and the cases leave out none (asserted): the rule of the Gaussian tests.
* everything else (scale 0, host / device parameters, in place, batch independence, two runs) is bit for bit.

Every bounded case prints its figure before it asserts."""
import random

import numpy as np
import pytest
import torch

import poisson_restatement as P
from dcpt_amd.keyed_init import keyed_input
from poisson_cases import CASES, case_args

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _host(v):
    return None if v is None else v.tolist()


_REF = {}


def reference(name, unit_scale=False, **flags):
    """the restatement's result for a case and flag set: computed once, shared, never modified"""
    k = (name, unit_scale, tuple(sorted(flags.items())))
    if k not in _REF:
        x, scale, key, gray = case_args(name)
        r = P.poisson_noise(x.numpy(), np.ones(len(scale), np.float32) if unit_scale else scale.numpy(), key.tolist(), _host(gray), **flags)
        excluded = int(r.near_level.sum()) + int(r.near_u.sum())
        assert excluded == 0, f"{name}: the restatement excludes {excluded} elements; choose other keys or inputs"
        for a in (r.T, r.k, r.lev, r.vals, r.U):
            a.setflags(write=False)
        _REF[k] = r
    return _REF[k]


def _within(y, t, what):
    d = np.abs(y.double().numpy() - t)
    bound = EPS32 * np.abs(t) + 1e-12
    worst = float((d / bound).max())
    print(f"{what}: max |y - T| {float(d.max()):.3e}; worst |y - T| / (2^-24 |T| + 1e-12) = {worst:.3f} over {d.size} elements")
    assert np.isfinite(y.numpy()).all() and worst <= 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_restatement(name, dev):
    """vals, the count of every element, and the out-of-place, in-place and noise_only outputs, with host and with device parameters: two
    launches a call"""
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    x, scale, key, gray = case_args(name)
    xd = x.to(dev)
    gd = None if gray is None else gray.to(dev)
    with kernel_trace() as t:
        y, vals = DF.poisson_noise(xd, scale, key, gray, return_vals=True)
        y2 = DF.poisson_noise(xd, scale.to(dev), key.to(dev), gd)
        z = xd.clone()
        zr = DF.poisson_noise(z, scale, key, gray, out=z)
        n = DF.poisson_noise(xd, scale, key, gray, noise_only=True)
        n1 = DF.poisson_noise(xd, 1.0, key, gray, noise_only=True)
    assert t.counts == {"noise.poisson_levels": 5, "noise.poisson": 5}, t.counts
    ref = reference(name)
    print(f"poisson_noise {name}: vals {vals.tolist()} against {ref.vals.tolist()} (U {ref.U.tolist()})")
    assert vals.dtype == torch.int32 and vals.is_cuda and vals.tolist() == ref.vals.tolist()
    # the count of every element
    one = reference(name, unit_scale=True, noise_only=True)
    f = (n1.cpu().double().numpy() + one.lev / 255.0) * one.vals.reshape(-1, 1, 1, 1)
    k = np.rint(f)
    print(f"poisson_noise {name}: {int((k != one.k).sum())} of {k.size} counts differ from the restatement's; largest k {int(one.k.max())}; "
          f"largest distance of the recovered value from an integer {float(np.abs(f - k).max()):.2e}")
    assert float(np.abs(f - k).max()) < 1e-3 and np.array_equal(k, one.k)
    assert y.dtype == torch.float32 and y.shape == x.shape and y.is_contiguous() and y.data_ptr() != xd.data_ptr()
    assert torch.equal(_bits(xd.cpu()), _bits(x))                               # out of place: x untouched
    assert zr.data_ptr() == z.data_ptr()
    _within(y.cpu(), ref.T, f"poisson_noise {name}")
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(z), _bits(y))   # device parameters and in place: the same bits
    _within(n.cpu(), reference(name, noise_only=True).T, f"poisson_noise {name} noise_only")
    if x.shape[1] == 3 and name not in ("zeros", "1x3x1x1"):
        for b in range(x.shape[0]):
            same = bool(torch.equal(n1[b, 0], n1[b, 1]) and torch.equal(n1[b, 0], n1[b, 2]))
            assert same == bool(gray is not None and gray[b]), (b, same)          # gray: one plane of noise; colour: not
    if name == "zeros":
        assert bool((n1 == 0).all()) and bool((y == 0).all())


def test_scale_zero_returns_x_bit_for_bit(dev):
    from dcpt_amd import functional as DF

    x, scale, key, gray = case_args("3x3x17x33")
    x[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, 1e-42, -3.5])
    y = DF.poisson_noise(x.to(dev), scale, key, gray).cpu()
    assert float(scale[0]) == 0.0 and torch.equal(_bits(y[0]), _bits(x[0])) and not torch.equal(y[1], x[1])
    y = DF.poisson_noise(x.to(dev), 0.0, 77, 1).cpu()
    assert torch.equal(_bits(y), _bits(x))
    assert bool((DF.poisson_noise(x.to(dev), 0.0, 77, noise_only=True) == 0).all())


@pytest.mark.parametrize("name", ["2x3x5x7", "3x3x17x33", "2x3x64x65"])
def test_clip_and_round8(name, dev):
    """(not the palettes: x = l / 255 makes 255 T = 255 k / vals up to the fp32 rounding of x, a half-integer for k = vals / 2, so the
    near-half rule would leave out a good part of them)"""
    from dcpt_amd import functional as DF

    x, scale, key, gray = case_args(name)
    xd = x.to(dev)
    y = DF.poisson_noise(xd, scale, key, gray, clip=True).cpu()
    _within(y, reference(name, clip=True).T, f"poisson_noise {name} clip")
    assert float(y.min()) == 0.0 and float(y.max()) == 1.0
    for clip in (False, True):
        y = DF.poisson_noise(xd, scale, key, gray, clip=clip, rounds=True).cpu()
        out = P.near_half(reference(name, clip=clip).T)
        assert int(out.sum()) == 0, f"{name}: the restatement leaves out {int(out.sum())} elements near a half-integer; choose other keys"
        want = reference(name, clip=clip, rounds=True).T
        v = y.double().numpy() * 255.0
        on_grid = np.abs(v - np.rint(v)) < 1e-3                     # (fp32 k / 255 times 255: within 2^-24 * |v| of the integer k, |v| < 1000)
        wrong = (y.numpy() != want.astype(np.float32)) & ~out
        print(f"poisson_noise {name} rounds clip={clip}: {int(wrong.sum())} of {y.numel()} differ from the restatement, {int((~on_grid).sum())} "
              f"off the 8-bit grid, {int(out.sum())} left out (cap {y.numel() // 1000})")
        assert int(out.sum()) <= y.numel() // 1000 and bool(on_grid.all()) and int(wrong.sum()) == 0
        if clip:
            assert 0.0 <= float(y.min()) and float(y.max()) <= 1.0


def test_an_image_does_not_depend_on_its_batch(dev):
    """image b of a batch equals the same image run alone and at another batch position, bit for bit; two runs give the same bits"""
    from dcpt_amd import functional as DF

    for name in ("2x3x5x7", "3x3x17x33"):
        x, scale, key, gray = case_args(name)
        xd = x.to(dev)
        y, vals = DF.poisson_noise(xd, scale, key, gray, return_vals=True)
        again, vals2 = DF.poisson_noise(xd, scale, key, gray, return_vals=True)
        assert torch.equal(_bits(again), _bits(y)) and torch.equal(vals, vals2)
        B = x.shape[0]
        for b in range(B):
            alone, v = DF.poisson_noise(xd[b:b + 1], scale[b:b + 1], key[b:b + 1], gray[b:b + 1], return_vals=True)
            assert torch.equal(_bits(alone[0]), _bits(y[b])) and int(v[0]) == int(vals[b]), (name, b)
        perm = list(range(B))[::-1] + [0]                           # reversed, and image 0 once more at the end of a longer batch
        idx = torch.tensor(perm)
        moved = DF.poisson_noise(xd[idx.to(dev)], scale[idx], key[idx], gray[idx])
        for pos, b in enumerate(perm):
            assert torch.equal(_bits(moved[pos]), _bits(y[b])), (name, pos, b)


def test_outputs_and_workspace_stay_inside_their_buffers(dev):
    """the entry point on an output and a workspace of exactly the size they need, with a guard behind each, at the misaligned and ragged
    shapes; both start as a NaN pattern, so an element the kernel skipped, or a mask it read without writing it, would show"""
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    with redzone() as rz:
        for name in ("1x3x1x1", "2x3x5x7", "3x3x17x33", "2x3x64x65"):
            x, scale, key, gray = case_args(name)
            B, C, H, W = x.shape
            for flags, ref in ((0, reference(name)), (4, reference(name, noise_only=True))):
                buf = DF._workspace(dev, 4 * x.numel())
                nws = lib.dcpt_poisson_noise_ws_bytes(B, C, H, W)
                ws = DF._workspace(dev, nws)
                DF._call(lib.dcpt_poisson_noise_fwd, (x.to(dev), scale.to(dev), key.to(dev), None if gray is None else gray.to(dev), buf, ws, nws),
                         (B, C, H, W, flags), dev)
                _within(buf.view(torch.float32).reshape(x.shape).cpu(), ref.T, f"red zone {name} flags={flags}")
                assert ws[:4 * B].view(torch.int32).tolist() == ref.vals.tolist()
            # the Python op takes its workspace from the same allocator
            y, vals = DF.poisson_noise(x.to(dev), scale, key, gray, return_vals=True)
            assert vals.tolist() == reference(name).vals.tolist()
    assert rz.count == 4 * 5


def test_refusals_of_the_python_op(dev):
    from dcpt_amd import functional as DF

    x = keyed_input("gpupoisson.bad", (2, 3, 8, 8)).to(dev)
    with pytest.raises(ValueError, match="negative"):
        DF.poisson_noise(x, -1.0, 1)
    with pytest.raises(ValueError, match="negative"):
        DF.poisson_noise(x, torch.tensor([0.5, -0.5]), 1)
    with pytest.raises(ValueError, match="poisson_noise: scale"):
        DF.poisson_noise(x, torch.tensor([0.5, 0.5, 0.5]), 1)
    with pytest.raises(ValueError, match="key"):
        DF.poisson_noise(x, 1.0, torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="64 bits"):
        DF.poisson_noise(x, 1.0, 1 << 64)
    with pytest.raises(ValueError):
        DF.poisson_noise(x[0], 1.0, 1)
    with pytest.raises(ValueError, match="out"):
        DF.poisson_noise(x, 1.0, 1, out=torch.empty((2, 3, 8, 9), device=dev))
    with pytest.raises(ValueError, match="1 or 3 channels"):
        DF.poisson_noise(keyed_input("gpupoisson.bad4", (2, 4, 8, 8)).to(dev), 1.0, 1, gray=1)
    with pytest.raises(NotImplementedError, match="inference-only"):
        DF.poisson_noise(x.clone().requires_grad_(True), 1.0, 1)
    # four channels without gray noise are fine; a device scale is not read back; a strided input is made contiguous; one key for every
    # image gives images with the same values the same noise
    assert DF.poisson_noise(keyed_input("gpupoisson.bad4", (2, 4, 8, 8)).to(dev), 1.0, 1).shape == (2, 4, 8, 8)
    same = x[:1].expand(2, 3, 8, 8)
    y = DF.poisson_noise(same.transpose(2, 3), torch.tensor([1.0, 1.0], device=dev), 9, noise_only=True)
    assert y.is_contiguous() and torch.equal(y[0], y[1]) and float(y.abs().max()) > 0


# ---- the reference's public functions ------------------------------------------------------------------
def test_the_pt_functions(dev):
    from kernel_trace import kernel_trace

    from basicsr.data import degradations as G

    img = keyed_input("gpupoisson.pt", (3, 3, 9, 11)).to(dev)
    gray = torch.tensor([0.0, 1.0, 0.0])
    with kernel_trace() as t:
        noise = G.generate_poisson_noise_pt(img, 1.0, gray, key=5)
    assert t.counts == {"noise.poisson_levels": 1, "noise.poisson": 1}, t.counts     # one call is two launches
    with kernel_trace() as t:
        out = G.add_poisson_noise_pt(img, 1.0, clip=False, rounds=False, gray_noise=gray, key=5)
    assert t.counts == {"noise.poisson_levels": 1, "noise.poisson": 1}, t.counts
    # image b uses key + b: the restatement with those keys
    ref = P.poisson_noise(img.cpu().numpy(), [1.0] * 3, [5, 6, 7], [0, 1, 0], noise_only=True)
    assert int(ref.near_level.sum()) + int(ref.near_u.sum()) == 0
    _within(noise.cpu(), ref.T, "generate_poisson_noise_pt")
    _within(out.cpu(), P.poisson_noise(img.cpu().numpy(), [1.0] * 3, [5, 6, 7], [0, 1, 0]).T, "add_poisson_noise_pt")
    assert torch.equal(noise[1, 0], noise[1, 1]) and torch.equal(noise[1, 0], noise[1, 2]) and not torch.equal(noise[0, 0], noise[0, 1])
    assert torch.equal(G.generate_poisson_noise_pt(img[2:], 1.0, 0, key=7), noise[2:])
    # scale as a per-image tensor, on the host or the device; a scalar gray_noise for every image
    per = G.generate_poisson_noise_pt(img, torch.tensor([1.0, 1.0, 1.0], device=dev), gray.to(dev), key=5)
    assert torch.equal(per, noise)
    assert torch.equal(G.generate_poisson_noise_pt(img, 1.0, 1, key=5)[1], noise[1])
    half = G.generate_poisson_noise_pt(img, 0.5, gray, key=5)
    assert torch.equal(half, 0.5 * noise)                                           # (a power of two: exact)
    # clip and rounds as in the reference
    c = G.add_poisson_noise_pt(img, 4.0, key=5)
    assert float(c.min()) == 0.0 and float(c.max()) == 1.0
    r = G.add_poisson_noise_pt(img, 4.0, clip=True, rounds=True, key=5) * 255
    assert bool(((r - r.round()).abs() < 1e-4).all()) and 0 <= float(r.min()) and float(r.max()) <= 255
    # key=None: torch.manual_seed governs the noise, the random_* draws included
    for fn in (lambda: G.generate_poisson_noise_pt(img, 1.0), lambda: G.add_poisson_noise_pt(img, 1.0, gray_noise=gray),
               lambda: G.random_generate_poisson_noise_pt(img, (0.05, 3.0), 0.5), lambda: G.random_add_poisson_noise_pt(img, (0.05, 3.0), 0.5, clip=False)):
        torch.manual_seed(123)
        a = fn()
        b = fn()
        torch.manual_seed(123)
        a2 = fn()
        assert torch.equal(_bits(a), _bits(a2)) and not torch.equal(a, b) and a.shape == img.shape
    torch.manual_seed(4)
    n = G.random_generate_poisson_noise_pt(img.repeat(8, 1, 1, 1), (1.0, 1.0), 0.5)
    grays = [bool(torch.equal(n[b, 0], n[b, 1])) for b in range(24)]
    # the noise of a pixel has the variance q / vals: its mean over a uniform image on 0..1 is 1 / (2 vals)
    std = float(n.std())
    print(f"random_generate_poisson_noise_pt: {sum(grays)} of 24 images gray at gray_prob 0.5; noise std {std:.4f} at scale 1")
    assert 0 < sum(grays) < 24 and 0.02 < std < 0.2


# ---- the data set and the models' feed_data ---------------------------------------------------------------
@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("poisson_gt")
    for i, (h, w) in enumerate([(40, 48), (33, 37), (48, 35), (36, 36)]):
        low = keyed_input(f"gpupoisson.png{i}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
        img = (img + keyed_input(f"gpupoisson.png{i}.n", (3, h, w), lo=-0.05, hi=0.05)).clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / f"im{i}.png")
    return str(root)


def test_feed_data_on_a_poisson_batch(png_folder, dev):
    """a ``noise_type: poisson`` batch through the train loader: two launches, the restatement's lq, clipped; a validation set shows the
    same noise on every visit"""
    from kernel_trace import kernel_trace

    from basicsr.data import build_dataloader, build_dataset
    from tests.test_gpu_jpeg import _sr_model

    model = _sr_model()
    kind = "PairedImageDenoiseDataset"
    ds = build_dataset(dict(name=kind, type=kind, dataroot_gt=png_folder, phase="train", gt_size=32, use_hflip=True, use_rot=True,
                            noise_type="poisson", noise_backend="device", poisson_scale=[0.5, 2.0], gray_prob=0.5))
    random.seed(5)
    torch.manual_seed(5)
    batch = next(iter(build_dataloader(ds, dict(phase="train", batch_size_per_gpu=4, num_worker_per_gpu=0))))
    assert "lq" not in batch and "degrade_kind" not in batch and tuple(batch["noise_key"].shape) == (4,)
    with kernel_trace() as t:
        model.feed_data(batch)
    assert t.counts == {"noise.poisson_levels": 1, "noise.poisson": 1}, t.counts
    want = P.poisson_noise(batch["gt"].numpy(), batch["poisson_scale"].numpy(), batch["noise_key"].tolist(), batch["poisson_gray"].tolist(), clip=True)
    assert int(want.near_level.sum()) + int(want.near_u.sum()) == 0
    print(f"feed_data on a Poisson batch: scale {batch['poisson_scale'].tolist()}, gray {batch['poisson_gray'].tolist()}, vals {want.vals.tolist()}")
    _within(model.lq.cpu(), want.T, "feed_data on a Poisson batch")
    assert torch.equal(model.gt.cpu(), batch["gt"]) and 0.0 <= float(model.lq.min()) and float(model.lq.max()) <= 1.0   # clipped
    assert not torch.equal(model.lq, model.gt)
    val = build_dataset(dict(name=kind, type=kind, dataroot_gt=png_folder, phase="val", noise_type="poisson", noise_backend="device",
                             poisson_scale=1.0, noise_seed=3))
    seen = []
    for _ in range(2):
        model.feed_data(next(iter(build_dataloader(torch.utils.data.Subset(val, [1]), dict(phase="val")))))
        seen.append(model.lq.clone())
    assert torch.equal(_bits(seen[0]), _bits(seen[1])) and tuple(seen[0].shape) == (1, 3, 33, 37)
