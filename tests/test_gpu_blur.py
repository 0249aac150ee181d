"""GPU: the blur kernel of dcpt_amd/csrc/blur.hip (through dcpt_amd.functional.filter2d, basicsr.utils.filter2D / USMSharp, the ``device``
backend of PairedImageBlurDataset, mixed batches of basicsr.data.degrade_collate and the models' ``feed_data``) against
tests/blur_restatement.py, the kernel-blind float64 numpy restatement of the header's arithmetic.

Everything is bit for bit (``torch.equal`` on the int32 views): each output is one float64 sum over the K * K taps in a stated order, every
step of which rounds once whether fused or not, rounded once to fp32, so the restatement rounded to fp32 IS the kernel's result.  The one
bounded check is ``USMSharp.forward`` against the reference's recorded output, ``2 K^2 2^-24`` (tests/test_blur_cpu.py derives it).

The kernel's output tile is T_H x T_W = 32 x 64; the shapes are the smallest at which it can go wrong: K = 1; K = 3 on 2 x 2 (both halos
reflect across the whole image); K = 21 at its least H, 11, one tile wide (11 x 11) and with W = 40; K = 51 at its least size 26 x 26 and
on 26 x (T_W + 1); (T_H + 1) x (T_W + 1) and (2 T_H - 1) x (T_W - 1) at K = 7, the ragged last tiles; C = 1 and 3; B = 3 with three
different random kernels (no symmetry: a flipped or transposed tap order, or a wrong image's kernel, fails); the shared (1, K, K) form;
a non-contiguous x; inputs in -0.5 .. 1.5."""
import os
import random

import numpy as np
import pytest
import torch

import blur_restatement as R
from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
T_H, T_W = 32, 64
# name -> (shape, K, one kernel per image)
CASES = {
    "k3_2x2": ((1, 3, 2, 2), 3, True),
    "k21_11x11_c1": ((1, 1, 11, 11), 21, True),
    "k21_11x40_b3": ((3, 3, 11, 40), 21, True),
    "k21_11x40_shared": ((3, 3, 11, 40), 21, False),
    "k51_26x26": ((1, 3, 26, 26), 51, True),
    "k51_26x65_c1": ((2, 1, 26, T_W + 1), 51, True),
    "k7_33x65": ((2, 3, T_H + 1, T_W + 1), 7, True),
    "k7_63x63": ((1, 3, 2 * T_H - 1, T_W - 1), 7, True),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _args(name):
    shape, K, per_image = CASES[name]
    x = keyed_input(f"gpublur.{name}", shape, lo=-0.5, hi=1.5)            # (negative values and values above 1)
    kern = keyed_input(f"gpublur.{name}.k", (shape[0] if per_image else 1, K, K), lo=-0.5, hi=1.0)
    return x, kern


_REF = {}


def reference(name):
    """the restatement rounded to fp32 for a case: computed once, shared, never modified"""
    if name not in _REF:
        x, kern = _args(name)
        _REF[name] = R.filter2d_f32(x.numpy(), kern.numpy())
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_restatement_bit_for_bit(name, dev):
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    x, kern = _args(name)
    xd = x.to(dev)
    with kernel_trace() as t:
        y = DF.filter2d(xd, kern)
        y2 = DF.filter2d(xd, kern.double().to(dev))     # any float dtype, any device
    assert t.counts == {"degrade.filter2d": 2}, t.counts
    assert y.dtype == torch.float32 and y.shape == x.shape and y.is_contiguous() and y.data_ptr() != xd.data_ptr()
    assert torch.equal(_bits(xd.cpu()), _bits(x))        # x untouched
    want = reference(name)
    differ = int((_bits(y.cpu()) != _bits(want)).sum())
    print(f"filter2d {name}: {differ} of {want.numel()} elements differ from the restatement; max |d| {float((y.cpu() - want).abs().max()):.3e}")
    assert differ == 0
    assert torch.equal(_bits(y2), _bits(y))              # two runs, the same bits
    if CASES[name][0][0] > 1 and CASES[name][2]:
        assert not torch.equal(y[0], DF.filter2d(xd[:1], kern[1:2])[0])   # the kernels of the images do differ


def test_identity_kernel_returns_x_bit_for_bit(dev):
    from dcpt_amd import functional as DF

    x = keyed_input("gpublur.identity", (2, 3, 5, 7), lo=-2.0, hi=2.0)
    x[0, 0, 0, :3] = torch.tensor([1e-42, 3.0e38, -1e-30])
    y = DF.filter2d(x.to(dev), torch.ones(1, 1, 1))
    assert torch.equal(_bits(y.cpu()), _bits(x))
    delta = torch.zeros(2, 5, 5)
    delta[:, 2, 2] = 1.0
    assert torch.equal(_bits(DF.filter2d(x.to(dev), delta).cpu()), _bits(x))
    # an off-centre delta shifts the reflect-padded image: the tap order is (dy, dx) = (row, column), no flip
    delta = torch.zeros(1, 3, 3)
    delta[0, 0, 2] = 1.0                                    # y[i][j] = xpad[i + 0][j + 2] = x[refl(i - 1)][refl(j + 1)]
    y = DF.filter2d(x.to(dev), delta).cpu()
    rows, cols = [1, 0, 1, 2, 3], [1, 2, 3, 4, 5, 6, 5]
    assert torch.equal(_bits(y), _bits(x[:, :, rows][:, :, :, cols]))


def test_a_non_contiguous_input(dev):
    from dcpt_amd import functional as DF

    x, kern = _args("k7_33x65")
    xd = x.to(dev)
    wide = torch.empty((2, 3, T_H + 1, 2 * (T_W + 1)), device=dev)
    wide[..., ::2] = xd
    wide[..., 1::2] = 7.0
    view = wide[..., ::2]
    assert not view.is_contiguous()
    assert torch.equal(_bits(DF.filter2d(view, kern).cpu()), _bits(reference("k7_33x65")))
    t = xd.transpose(2, 3)                                   # (2, 3, 65, 33), strided
    assert torch.equal(_bits(DF.filter2d(t, kern).cpu()), _bits(R.filter2d_f32(x.transpose(2, 3).contiguous().numpy(), kern.numpy())))


def test_outputs_stay_inside_their_buffers(dev):
    """the entry point on outputs of exactly the size they need, with a guard behind them (and the previous allocation's guard in front),
    at the least-H shapes; the outputs start as a NaN pattern, so an element the kernel skipped would show"""
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    with redzone() as rz:
        for name in ("k21_11x40_b3", "k51_26x26"):
            x, kern = _args(name)
            B, C, H, W = x.shape
            buf = DF._workspace(dev, 4 * x.numel())
            DF._call(lib.dcpt_filter2d_fwd, (x.to(dev), kern.to(dev), buf), (B, C, H, W, kern.shape[-1], 1), dev)
            assert torch.equal(_bits(buf.view(torch.float32).reshape(x.shape).cpu()), _bits(reference(name))), name
    assert rz.count == 2


def test_refusals_of_the_python_op(dev):
    from dcpt_amd import functional as DF

    x = keyed_input("gpublur.bad", (2, 3, 8, 8)).to(dev)
    for kern, text in [(torch.ones(2, 4, 4), "odd"), (torch.ones(3, 3, 3), "kernel must be"), (torch.ones(2, 3, 5), "kernel must be"),
                       (torch.ones(3, 3), "kernel must be"), (torch.ones(2, 3, 3, dtype=torch.int32), "kernel must be"),
                       (torch.ones(1, 17, 17), "reflect padding"), (torch.ones(1, 53, 53), "odd")]:
        with pytest.raises(ValueError, match=text):
            DF.filter2d(x, kern)
    with pytest.raises(ValueError, match="reflect padding"):
        DF.filter2d(x[:, :, :, :1], torch.ones(1, 3, 3))
    with pytest.raises(ValueError):
        DF.filter2d(x[0], torch.ones(1, 3, 3))
    with pytest.raises(NotImplementedError, match="inference-only"):
        DF.filter2d(x.clone().requires_grad_(True), torch.ones(1, 3, 3))


# ---- the reference's public surface ------------------------------------------------------------------------
def test_filter2D_and_usmsharp_equal_the_cpu_expressions_around_the_restated_blur(dev, golden_dir):
    from kernel_trace import kernel_trace

    from basicsr.utils import USMSharp, filter2D

    z = np.load(os.path.join(golden_dir, "filter2d.npz"))
    for tag in ("per_image", "shared", "tiny"):
        x, kern = torch.from_numpy(z[f"{tag}.x"]), torch.from_numpy(z[f"{tag}.kernel"])
        y = filter2D(x.to(dev), kern.to(dev)).cpu()
        assert torch.equal(_bits(y), _bits(R.filter2d_f32(x.numpy(), kern.numpy()))), tag
        K = kern.shape[-1]
        d = float((y.double() - torch.from_numpy(z[f"{tag}.y"]).double()).abs().max())
        print(f"filter2D {tag} against the reference's fp32 output: max |d| {d:.3e}, bound {K * K * 2.0 ** -24:.3e}")
        assert d <= K * K * 2.0 ** -24
    with pytest.raises(ValueError, match="Wrong kernel size"):
        filter2D(x.to(dev), torch.ones(1, 4, 4))
    radius, weight, threshold = z["usm.args"].tolist()
    img = torch.from_numpy(z["usm.x"])
    usm = USMSharp(int(radius)).to(dev)
    assert torch.equal(usm.kernel.cpu(), torch.from_numpy(z["usm.kernel"]))
    with kernel_trace() as t:
        out = usm(img.to(dev), weight=weight, threshold=threshold).cpu()
    assert t.counts == {"degrade.filter2d": 2}, t.counts
    want = R.usm_sharp(img, usm.kernel.cpu(), weight, threshold)
    assert torch.equal(_bits(out), _bits(want))
    d = float((out.double() - torch.from_numpy(z["usm.y"]).double()).abs().max())
    bound = 2 * radius * radius * 2.0 ** -24
    print(f"USMSharp.forward against the reference's output: max |d| {d:.3e}, bound {bound:.3e}")
    assert d <= bound
    # the default module: a 51 x 51 Gaussian
    big = keyed_input("gpublur.usm51", (1, 3, 40, 30))
    usm51 = USMSharp().to(dev)
    assert torch.equal(_bits(usm51(big.to(dev)).cpu()), _bits(R.usm_sharp(big, usm51.kernel.cpu())))


# ---- the data set, the models' feed_data and mixed batches ------------------------------------------------------
@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("blur_gt")
    for i, (h, w) in enumerate([(40, 48), (33, 37), (48, 35), (36, 36)]):
        low = keyed_input(f"gpublur.png{i}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
        img = (img + keyed_input(f"gpublur.png{i}.n", (3, h, w), lo=-0.05, hi=0.05)).clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / f"im{i}.png")
    return str(root)


def _set(kind, root, **over):
    from basicsr.data import build_dataset

    opt = dict(name=kind, type=kind, dataroot_gt=root, phase="train", gt_size=32, use_hflip=True, use_rot=True)
    opt.update(over)
    return build_dataset(opt)


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def test_feed_data_on_a_device_blur_batch_gives_the_host_backends_lq(png_folder, dev):
    from kernel_trace import kernel_trace

    from basicsr.data import degrade_collate
    from tests.test_gpu_jpeg import _sr_model

    host = _set("PairedImageBlurDataset", png_folder, blur_kernel_size=13)
    device = _set("PairedImageBlurDataset", png_folder, blur_kernel_size=13, blur_backend="device")
    samples, twins = [], []
    for i in range(4):
        _seed(900 + i)
        samples.append(device[i])
        _seed(900 + i)
        twins.append(host[i])
    batch = degrade_collate([dict(s) for s in samples])
    assert "lq" not in batch and "degrade_kind" not in batch and tuple(batch["blur_kernel"].shape) == (4, 13, 13)
    model = _sr_model()
    with kernel_trace() as t:
        model.feed_data(batch)
    assert t.counts == {"degrade.filter2d": 1}, t.counts
    want = torch.stack([s["lq"] for s in twins])
    assert torch.equal(model.gt.cpu(), batch["gt"]) and torch.equal(_bits(model.lq.cpu()), _bits(want))
    assert not torch.equal(model.lq, model.gt)


def test_feed_data_on_a_mixed_batch_of_noise_and_blur_rows(png_folder, dev):
    from kernel_trace import kernel_trace

    from basicsr.data import degrade_collate
    from dcpt_amd import functional as DF
    from tests.test_gpu_jpeg import _sr_model

    blur = _set("PairedImageBlurDataset", png_folder, blur_kernel_size=9, blur_backend="device")
    twin = _set("PairedImageBlurDataset", png_folder, blur_kernel_size=9)
    noise = _set("PairedImageDenoiseDataset", png_folder, sigma_type="choice", sigma_range=[15, 50], noise_backend="device")
    order, samples, twins = [1, 0, 1, 1, 0], [], []
    for i, k in enumerate(order):
        _seed(950 + i)
        samples.append((blur if k else noise)[i % 4])
        _seed(950 + i)
        twins.append(twin[i % 4] if k else None)
    batch = degrade_collate([dict(s) for s in samples])
    assert batch["degrade_kind"].tolist() == [5, 1, 5, 5, 1] and tuple(batch["blur_kernel"].shape) == (3, 9, 9)
    model = _sr_model()
    with kernel_trace() as t:
        model.feed_data(batch)
    assert t.counts == {"noise.gauss": 1, "degrade.filter2d": 1}, t.counts
    lq, gt = model.lq, batch["gt"].to(dev)
    rows = {k: [i for i, v in enumerate(batch["degrade_kind"].tolist()) if v == k] for k in (1, 5)}
    assert torch.equal(_bits(lq[rows[1]]), _bits(DF.gaussian_noise(gt[rows[1]], batch["noise_sigma"], batch["noise_key"])))
    assert torch.equal(_bits(lq[rows[5]]), _bits(DF.filter2d(gt[rows[5]], batch["blur_kernel"])))
    for i in rows[5]:
        assert torch.equal(_bits(lq[i].cpu()), _bits(twins[i]["lq"])), i        # the host backend's lq
    assert bool(torch.isfinite(lq).all()) and all(not torch.equal(lq[i], gt[i]) for i in range(5))
