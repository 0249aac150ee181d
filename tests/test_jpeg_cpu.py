"""CPU: the yardstick of the DiffJPEG kernel (tests/jpeg_restatement.py against the golden vectors of the reference's DiffJPEG,
tests/golden/diffjpeg.npz, made by tools/make_golden_diffjpeg.py) and the surface that needs no device: quality_to_factor, the refusals of
dcpt_diffjpeg_fwd, PairedImageJPEGCARDataset on a temporary folder, and ``feed_data`` of a CPU model on a ``jpeg_backend: device`` batch.

The bound on the restatement, every element within 2e-6, is about six times the 3.5e-7 measured between the reference in fp32 and its own
float64 form; each case prints its figure before it asserts."""
import os
import random

import numpy as np
import pytest
import torch

import jpeg_restatement as R
from dcpt_amd.keyed_init import keyed_input
from tests import test_plumbing_cpu as TP   # registers the CPU stand-in arch ``_TestConvArch``

TOL = 2e-6
# tag -> shape: the cases of tools/make_golden_diffjpeg.py (qualities and the seed of the keyed input are stored with the vectors)
GOLDEN_CASES = {"mb3x2": (2, 3, 24, 40), "one_mb": (1, 3, 16, 16), "ragged": (2, 3, 17, 33), "grey": (2, 1, 24, 24), "pixel": (1, 3, 1, 1)}


def golden_case(golden_dir, tag):
    """(x, quality as a (B,) float32 tensor, hard output, soft output) of one golden case"""
    z = np.load(os.path.join(golden_dir, "diffjpeg.npz"))
    shape = GOLDEN_CASES[tag]
    x = keyed_input(f"diffjpeg.{tag}", shape, seed=int(z[f"{tag}.seed"]))
    q = torch.from_numpy(np.broadcast_to(z[f"{tag}.quality"], (shape[0],)).copy())
    return x, q, torch.from_numpy(z[f"{tag}.hard"]), torch.from_numpy(z[f"{tag}.soft"])


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_restatement_matches_the_reference_vectors(tag, golden_dir):
    x, q, hard, soft = golden_case(golden_dir, tag)
    assert tuple(hard.shape) == GOLDEN_CASES[tag] and tuple(soft.shape) == GOLDEN_CASES[tag]
    for name, want, diff in (("round", hard, False), ("diff_round", soft, True)):
        res = R.diffjpeg(x, q, differentiable=diff)
        d = float((res.y - want.double()).abs().max())
        print(f"restatement against the reference, {tag} {GOLDEN_CASES[tag]} q={q.tolist()} {name}: max |d| {d:.3e} (bound {TOL:.0e})")
        assert d <= TOL
        assert not R.tie_macroblocks(res, 1e-6)   # the committed keys hold no contested rounding
    assert float((hard - soft).abs().max()) > 1e-4   # the two roundings are different functions
    assert float((hard - x).abs().max()) > 1e-3 or tag == "pixel"   # and the codec is not the identity


def test_restatement_options():
    """uint8_io puts input and output on the 8-bit grid; a number and a tensor quality are the same thing; quality is not modified"""
    x = keyed_input("jpegcpu.opt", (2, 3, 17, 33))
    q = torch.tensor([30.0, 30.0])
    a, b = R.diffjpeg(x, q, uint8_io=True), R.diffjpeg(x, 30, uint8_io=True)
    assert torch.equal(a.y, b.y) and torch.equal(q, torch.tensor([30.0, 30.0]))
    assert torch.equal(torch.round(a.y * 255), torch.round(a.pre)) and float((a.y * 255 - torch.round(a.y * 255)).abs().max()) < 1e-12
    on_grid = torch.round(x * 255) / 255
    assert torch.equal(R.diffjpeg(on_grid.float(), q, uint8_io=True).y, a.y)
    g = R.diffjpeg(x[:, :1], q)
    assert tuple(g.y.shape) == (2, 1, 17, 33) and tuple(g.t_y.shape) == (2, 4, 6, 8, 8) and tuple(g.t_cb.shape) == (2, 2, 3, 8, 8)


def test_quality_to_factor():
    from basicsr.utils import quality_to_factor

    for q, want in [(10, 5.0), (49.9, 5000.0 / 49.9 / 100.0), (50, 1.0), (95, 0.1)]:
        assert quality_to_factor(q) == pytest.approx(want, rel=1e-15), q
        assert float(R.quality_to_factor(q)) == pytest.approx(want, rel=1e-15), q
    assert quality_to_factor(49.9) > 1.0 and quality_to_factor(50) == 1.0   # the two branches meet at 50


def test_imports_and_constructor():
    import inspect

    import basicsr.utils as U
    from basicsr.utils import DiffJPEG, quality_to_factor  # noqa: F401
    from basicsr.utils.diffjpeg import DiffJPEG as D2

    assert D2 is DiffJPEG and "DiffJPEG" in U.__all__ and "quality_to_factor" in U.__all__
    assert [(p.name, p.default) for p in inspect.signature(DiffJPEG.__init__).parameters.values()][1:] == [("differentiable", True)]
    assert list(inspect.signature(DiffJPEG.forward).parameters) == ["self", "x", "quality"]
    m = DiffJPEG()
    assert m.differentiable is True and not list(m.parameters()) and DiffJPEG(differentiable=False).differentiable is False


def test_entry_point_refuses_bad_arguments_without_a_device():
    """every check comes before the launch: each refusal is reported, with its text, on a machine with no GPU"""
    from kernel_trace import kernel_trace

    from dcpt_amd import _lib

    lib = _lib.load()
    f = lib.dcpt_diffjpeg_fwd
    with kernel_trace() as t:
        for args in [(None, 8, 8), (8, None, 8), (8, 8, None)]:
            assert f(*args, 1, 3, 16, 16, 0, None) == 1 and b"null" in lib.dcpt_last_error()
        for dims, text in [((1, 2, 16, 16), b"C must be 1 or 3"), ((1, 0, 16, 16), b"C must be 1 or 3"), ((1, 4, 16, 16), b"C must be 1 or 3"),
                           ((1, 3, 0, 16), b"bad shape"), ((1, 3, 16, 0), b"bad shape"), ((0, 3, 16, 16), b"bad shape"),
                           ((-1, 3, 16, 16), b"bad shape"), ((65536, 1, 1, 1), b"B above 65535"), ((1, 1, 1 << 16, 1 << 15), b"2^30 pixels")]:
            assert f(8, 8, 8, *dims, 0, None) == 1 and text in lib.dcpt_last_error(), (dims, lib.dcpt_last_error())
        assert f(8, 8, 8, 1, 3, 16, 16, 4, None) == 1 and b"unknown flags" in lib.dcpt_last_error()
    assert t.counts == {}, t.counts
    assert lib.dcpt_abi_version() == 16


def test_op_refuses_cpu_tensors():
    from basicsr.utils import DiffJPEG
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    x = keyed_input("jpegcpu.cpu", (1, 3, 8, 8))
    for call in (lambda: DF.diffjpeg(x, 30), lambda: DiffJPEG(differentiable=False)(x, 30), lambda: DF.diffjpeg(x, torch.tensor([30.0]))):
        with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
            call()
    with pytest.raises(_lib.DcptHipError):
        DF.diffjpeg(x.numpy(), 30)


# ---- the dataset ----------------------------------------------------------------------------------
NAMES = ["a.png", "b.png", "c.png"]
SIZES = {"a.png": (40, 48), "b.png": (33, 37), "c.png": (64, 35)}


@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("car_gt")
    for n in NAMES:
        h, w = SIZES[n]
        low = keyed_input(f"jpegcpu.{n}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
        img = (img + keyed_input(f"jpegcpu.{n}.n", (3, h, w), lo=-0.05, hi=0.05)).clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / n)
    (root / "notes.txt").write_text("not an image")
    return str(root)


def _set(root, **over):
    from basicsr.data import build_dataset

    opt = dict(name="car", type="PairedImageJPEGCARDataset", dataroot_gt=root, phase="val", q_type="constant", q_range=30)
    opt.update(over)
    return build_dataset(opt)


def test_dataset_is_registered_pairs_and_crops(png_folder):
    from basicsr.data import PairedImageJPEGCARDataset
    from basicsr.utils.registry import DATASET_REGISTRY

    assert DATASET_REGISTRY.get("PairedImageJPEGCARDataset") is PairedImageJPEGCARDataset
    ds = _set(png_folder, dataset_idx=4)
    assert isinstance(ds, PairedImageJPEGCARDataset) and len(ds) == 3
    for i, n in enumerate(NAMES):
        s = ds[i]
        assert s["gt_path"] == s["lq_path"] == os.path.join(png_folder, n) and s["dataset_idx"] == 4
        assert tuple(s["gt"].shape) == tuple(s["lq"].shape) == (3, *SIZES[n]) and s["gt"].dtype == s["lq"].dtype == torch.float32
    s = _set(png_folder, center_crop=32)[1]
    assert tuple(s["gt"].shape) == tuple(s["lq"].shape) == (3, 32, 32)
    random.seed(3)
    s = _set(png_folder, phase="train", gt_size=24, use_hflip=True, use_rot=True)[2]
    assert tuple(s["gt"].shape) == tuple(s["lq"].shape) == (3, 24, 24)
    assert _set(png_folder, phase="train", use_hflip=False, use_rot=False).gt_size == 128   # the default
    with pytest.raises(ValueError, match="smaller than the training patch"):
        _set(png_folder, phase="train", use_hflip=False, use_rot=False)[0]
    with pytest.raises(AssertionError):
        _set(png_folder, q_type="uniform")
    with pytest.raises(ValueError, match="jpeg_backend"):
        _set(png_folder, jpeg_backend="cv2")


def test_pil_backend_gives_an_8_bit_image_that_differs_from_gt(png_folder):
    ds10, ds90 = _set(png_folder, q_range=10), _set(png_folder, q_range=90)
    for i in range(3):
        a, b = ds10[i], ds90[i]
        for s in (a, b):
            v = s["lq"] * 255
            assert torch.equal(v, torch.round(v)) and 0 <= float(s["lq"].min()) and float(s["lq"].max()) <= 1
            assert "jpeg_quality" not in s
        e10, e90 = float((a["lq"] - a["gt"]).abs().mean()), float((b["lq"] - b["gt"]).abs().mean())
        assert torch.equal(a["gt"], b["gt"]) and e10 > e90 > 0 and e10 < 0.1   # artifacts, more of them at the lower quality


def test_quality_draws_replay_pythons_random(png_folder):
    """the draw is Python's ``random``, after the crop and the augmentation, exactly as the reference's :532-537"""
    dev = dict(jpeg_backend="device")
    for q_type, q_range, draw in [("constant", 35, lambda: 35), ("random", [10, 40], lambda: random.uniform(10, 40)),
                                  ("choice", [10, 20, 30, 40], lambda: random.choice([10, 20, 30, 40]))]:
        ds = _set(png_folder, q_type=q_type, q_range=q_range, **dev)
        random.seed(17)
        got = [float(ds[i % 3]["jpeg_quality"]) for i in range(9)]
        random.seed(17)
        want = [float(np.float32(draw())) for _ in range(9)]
        assert got == want, (q_type, got, want)
        assert q_type == "constant" or len(set(got)) > 1
    # the train phase: two crop offsets, three augmentation draws, then the quality
    ds = _set(png_folder, phase="train", gt_size=16, use_hflip=True, use_rot=True, q_type="choice", q_range=[10, 20, 30, 40], **dev)
    random.seed(5)
    got = [float(ds[i % 3]["jpeg_quality"]) for i in range(6)]
    random.seed(5)
    want = []
    for i in range(6):
        h, w = SIZES[NAMES[i % 3]]
        random.randint(0, h - 16), random.randint(0, w - 16)
        random.random(), random.random(), random.random()
        want.append(float(random.choice([10, 20, 30, 40])))
    assert got == want


def test_device_backend_sample_and_batch(png_folder):
    from basicsr.data import build_dataloader

    ds = _set(png_folder, jpeg_backend="device", q_type="choice", q_range=[10, 20, 30, 40], center_crop=32)
    s = ds[0]
    assert sorted(s) == ["gt", "gt_path", "jpeg_quality", "lq_path"]
    assert s["jpeg_quality"].dtype == torch.float32 and s["jpeg_quality"].dim() == 0 and float(s["jpeg_quality"]) in (10, 20, 30, 40)
    batch = next(iter(build_dataloader(ds, dict(phase="train", batch_size_per_gpu=2, num_worker_per_gpu=0))))
    assert tuple(batch["gt"].shape) == (2, 3, 32, 32) and tuple(batch["jpeg_quality"].shape) == (2,) and "lq" not in batch


def _cpu_model(model_type="SRModel"):
    from basicsr.models import build_model

    return build_model(TP._opt(model_type=model_type))


def test_feed_data_on_a_cpu_model_raises_the_no_cpu_fallback_error(png_folder):
    """a ``jpeg_backend: device`` batch reaches the DiffJPEG kernel in feed_data -- not a KeyError for the missing lq; a batch that carries
    lq takes the path it always took"""
    from dcpt_amd import _lib

    m = _cpu_model()
    gt = keyed_input("jpegcpu.feed", (2, 3, 16, 16))
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        m.feed_data({"gt": gt, "jpeg_quality": torch.tensor([10.0, 40.0])})
    lq = keyed_input("jpegcpu.feed.lq", (2, 3, 16, 16))
    m.feed_data({"lq": lq, "gt": gt, "jpeg_quality": torch.tensor([10.0, 40.0])})
    assert torch.equal(m.lq, lq) and torch.equal(m.gt, gt)
    with pytest.raises(KeyError):
        m.feed_data({"gt": gt})
