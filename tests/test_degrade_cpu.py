"""CPU: the yardstick of the demosaic and line-mask kernels (tests/degrade_restatement.py against the golden vectors of the reference's
basicsr/utils/mosaic_util.py, tests/golden/mosaic.npz, made by tools/make_golden_mosaic.py) and the surface that needs no device: the
refusals of dcpt_demosaic_fwd and dcpt_inpaint_lines_fwd, the host mosaic helpers, PairedImageMosaicDataset, PairedImageInpaintingDataset
and PairedImageDehazeDataset on temporary folders, and ``feed_data`` of a CPU model on device-backend batches.

The restatement is integer arithmetic and the reference's float64 outputs on 8-bit inputs are exact multiples of 1/16 (1/4), so the two
are compared for equality."""
import os
import random

import numpy as np
import pytest
import torch

import degrade_restatement as R
from dcpt_amd.keyed_init import keyed_input
from tests import test_plumbing_cpu as TP   # registers the CPU stand-in arch ``_TestConvArch``

# tag -> shape: the cases of tools/make_golden_mosaic.py
GOLDEN_CASES = {"4x4": (1, 3, 4, 4), "6x8": (1, 3, 6, 8), "16x16": (1, 3, 16, 16), "34x66": (1, 3, 34, 66), "b2_10x12": (2, 3, 10, 12)}
METHODS = {"malvar": 16, "bilinear": 4}


def golden_case(golden_dir, tag):
    """(the keyed [0, 1] input as float32 numpy, the arrays of the case by name)"""
    z = np.load(os.path.join(golden_dir, "mosaic.npz"))
    x = keyed_input(f"mosaic.{tag}", GOLDEN_CASES[tag]).numpy()
    return x, {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(tag + ".")}


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_restatement_equals_the_reference_vectors(tag, golden_dir):
    x, g = golden_case(golden_dir, tag)
    b, _, h, w = GOLDEN_CASES[tag]
    cfa = R.cfa_of(R.to_u8(x))
    assert g["cfa"].dtype == np.uint8 and g["cfa"].shape == (b, h, w) and np.array_equal(cfa, g["cfa"])   # the reference's own mosaic
    for method, unit in METHODS.items():
        s, u = R.sums(cfa, method)
        assert u == unit and s.dtype == np.int64 and np.array_equal(s, g[f"{method}64"] * unit)   # exact: difference 0
        d = float(np.abs(R.demosaic_f64(x, method) - g[f"{method}32"]).max())
        print(f"restatement in float64 against the reference in fp32, {tag} {method}: max |d| {d:.3e}")
        assert d <= 1.94e-6
    # the 8-bit cases are not soft: ties of the final rounding and sums outside 0..255 both occur
    s = R.malvar_sums(cfa)
    ties, outside = int((s % 16 == 8).sum()), int(((s < 0) | (s > 255 * 16)).sum())
    print(f"{tag}: {ties} rounding ties, {outside} sums outside 0..255")
    assert ties >= 1 and outside >= 1
    assert int((R.bilinear_sums(cfa) % 4 == 2).sum()) >= 1


def test_restatement_rounding_and_line_rule():
    s = np.array([8, 24, 40, -8, 7, 9, 255 * 16 + 8, 255 * 16 - 8, 300 * 16, -100])
    assert R.round_to_grid(s, 16).tolist() == [0, 2, 2, 0, 0, 1, 255, 254, 255, 0]   # half to even, then the clamp
    m = R.line_mask([[2, 2, 2, 2]] + [[0, 0, 0, 0]] * 9, [1, 4, 1], 5, 5)   # a zero-length stroke: a disc of radius 2
    assert m.sum() == 13 and m[2, 0] and m[0, 2] and not m[0, 0] and not m[1, 0]
    m = R.line_mask([[0, 3, 8, 3]] + [[0, 0, 0, 0]] * 9, [1, 2, 0], 7, 9)   # a horizontal stroke, thick 2: rows 2..4 of every column
    assert m[2:5].all() and not m[:2].any() and not m[5:].any()
    assert not R.line_mask(np.zeros((10, 4), int), [0, 5, 1], 4, 4).any()


def test_host_mosaic_helpers(golden_dir):
    import basicsr.utils as U
    from basicsr.utils import dm, dm_matlab, masks_CFA_Bayer, mosaic_CFA_Bayer  # noqa: F401
    from basicsr.utils import mosaic_util as M

    assert all(n in U.__all__ for n in ("masks_CFA_Bayer", "mosaic_CFA_Bayer", "dm", "dm_matlab")) and M.dm_matlab is dm_matlab
    r, g, b = masks_CFA_Bayer((3, 5))
    assert r.dtype == bool and r.tolist()[0] == [True, False, True, False, True] and not r[1].any()
    assert b[1].tolist() == [False, True, False, True, False] and np.array_equal(g, ~(r | b)) and g[0, 1] and g[1, 0]
    for tag in ("6x8", "b2_10x12"):
        x, gold = golden_case(golden_dir, tag)
        u8 = np.rint(x * 255).astype(np.uint8)
        for i in range(x.shape[0]):
            hwc = u8[i].transpose(1, 2, 0)
            cfa, cfa4, mosaic, mask = mosaic_CFA_Bayer(hwc)
            assert cfa.dtype == np.uint8 and np.array_equal(cfa, gold["cfa"][i])
            assert cfa4.dtype == np.uint8 and cfa4.shape == (hwc.shape[0] // 2, hwc.shape[1] // 2, 4)
            assert np.array_equal(cfa4[:, :, 1], cfa[0::2, 1::2]) and np.array_equal(cfa4[:, :, 2], cfa[1::2, 0::2])
            assert mask.dtype == bool and mask.shape == hwc.shape and np.array_equal(mosaic, hwc * mask) and (mask.sum(2) == 1).all()
    with pytest.raises(ValueError, match="even"):
        mosaic_CFA_Bayer(np.zeros((5, 4, 3), np.uint8))


def test_entry_points_refuse_bad_arguments_without_a_device():
    """every check comes before the launch: each refusal is reported, with its text, on a machine with no GPU"""
    from kernel_trace import kernel_trace

    from dcpt_amd import _lib

    lib = _lib.load()
    f, g = lib.dcpt_demosaic_fwd, lib.dcpt_inpaint_lines_fwd
    with kernel_trace() as t:
        for args in [(None, 16), (16, None)]:
            assert f(*args, 1, 3, 8, 8, 0, None) == 1 and b"null" in lib.dcpt_last_error()
        assert f(16, 16, 1, 3, 8, 8, 0, None) == 1 and b"different buffers" in lib.dcpt_last_error()
        for dims, text in [((1, 2, 8, 8), b"C must be 1 or 3"), ((1, 0, 8, 8), b"C must be 1 or 3"), ((1, 4, 8, 8), b"C must be 1 or 3"),
                           ((1, 3, 2, 8), b"at least 3"), ((1, 3, 8, 2), b"at least 3"), ((1, 1, 0, 8), b"at least 3"),
                           ((0, 3, 8, 8), b"B outside 1..65535"), ((-1, 3, 8, 8), b"B outside 1..65535"),
                           ((65536, 1, 3, 3), b"B outside 1..65535"), ((1, 1, 1 << 16, 1 << 15), b"2^30 pixels")]:
            assert f(16, 32, *dims, 0, None) == 1 and text in lib.dcpt_last_error(), (dims, lib.dcpt_last_error())
        for flags in (4, 8, -1):
            assert f(16, 32, 1, 3, 8, 8, flags, None) == 1 and b"unknown flags" in lib.dcpt_last_error()

        for args in [(None, 8, 8, 8), (8, None, 8, 8), (8, 8, None, 8), (8, 8, 8, None)]:
            assert g(*args, 1, 3, 8, 8, None) == 1 and b"null" in lib.dcpt_last_error()
        for dims, text in [((0, 3, 8, 8), b"bad shape"), ((-1, 3, 8, 8), b"bad shape"), ((1, 3, 0, 8), b"bad shape"), ((1, 3, 8, 0), b"bad shape"),
                           ((1, 2, 8, 8), b"C must be 1 or 3"), ((1, 4, 8, 8), b"C must be 1 or 3"), ((1, 3, 16385, 8), b"above 16384"),
                           ((1, 1, 8, 16385), b"above 16384"), ((65536, 1, 1, 1), b"B above 65535")]:
            assert g(8, 8, 8, 8, *dims, None) == 1 and text in lib.dcpt_last_error(), (dims, lib.dcpt_last_error())
    assert t.counts == {}, t.counts


def test_header_and_ctypes_table_carry_both_names():
    from dcpt_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dcpt_hip.h")).read()
    for name in ("dcpt_demosaic_fwd", "dcpt_inpaint_lines_fwd"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert "#define DCPT_DEMOSAIC_BILINEAR 1" in header and "#define DCPT_DEMOSAIC_UINT8_IO 2" in header
    assert _lib.load().dcpt_abi_version() == 16


def test_ops_refuse_cpu_tensors():
    from basicsr.utils import dm, dm_matlab
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    x = keyed_input("degradecpu.cpu", (1, 3, 8, 8))
    lines, meta = torch.zeros((1, 10, 4), dtype=torch.int32), torch.tensor([[1, 5, 1]], dtype=torch.int32)
    pack = keyed_input("degradecpu.pack", (1, 4, 4, 4))
    for call in (lambda: DF.demosaic(x), lambda: DF.demosaic(x[:, :1], "bilinear", uint8_io=True), lambda: DF.inpaint_lines(x, lines, meta),
                 lambda: dm(pack), lambda: dm_matlab(pack)):
        with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
            call()
    with pytest.raises(_lib.DcptHipError):
        DF.demosaic(x.numpy())
    with pytest.raises(_lib.DcptHipError):
        DF.inpaint_lines(x.numpy(), lines, meta)


# ---- the datasets -----------------------------------------------------------------------------------
NAMES = ["a.png", "b.png", "c.png"]
SIZES = {"a.png": (40, 48), "b.png": (33, 37), "c.png": (64, 35)}


def _save(img, path):
    from PIL import Image

    Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(path)


def _image(tag, h, w):
    low = keyed_input(tag, (1, 3, h // 4 + 1, w // 4 + 1))
    img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
    return (img + keyed_input(tag + ".n", (3, h, w), lo=-0.05, hi=0.05)).clamp(0, 1)


@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("degrade_gt")
    for n in NAMES:
        _save(_image(f"degradecpu.{n}", *SIZES[n]), root / n)
    (root / "notes.txt").write_text("not an image")
    return str(root)


def _set(kind, root, **over):
    from basicsr.data import build_dataset

    opt = dict(name=kind, type=kind, dataroot_gt=root, phase="val")
    opt.update(over)
    return build_dataset(opt)


MOSAIC, INPAINT = "PairedImageMosaicDataset", "PairedImageInpaintingDataset"


@pytest.mark.parametrize("kind", [MOSAIC, INPAINT])
def test_datasets_are_registered_pair_and_crop(kind, png_folder):
    import basicsr.data as D
    from basicsr.utils.registry import DATASET_REGISTRY

    assert DATASET_REGISTRY.get(kind) is getattr(D, kind)
    ds = _set(kind, png_folder, dataset_idx=6)
    assert isinstance(ds, getattr(D, kind)) and len(ds) == 3 and ds.backend == "host"
    for i, n in enumerate(NAMES):
        s = ds[i]
        assert s["gt_path"] == s["lq_path"] == os.path.join(png_folder, n) and s["dataset_idx"] == 6
        assert tuple(s["gt"].shape) == tuple(s["lq"].shape) == (3, *SIZES[n]) and s["gt"].dtype == s["lq"].dtype == torch.float32
        assert not torch.equal(s["gt"], s["lq"])
    s = _set(kind, png_folder, center_crop=32)[1]
    assert tuple(s["gt"].shape) == tuple(s["lq"].shape) == (3, 32, 32)
    random.seed(3)
    s = _set(kind, png_folder, phase="train", gt_size=24, use_hflip=True, use_rot=True)[2]
    assert tuple(s["gt"].shape) == tuple(s["lq"].shape) == (3, 24, 24)
    assert _set(kind, png_folder, phase="train", use_hflip=False, use_rot=False).gt_size == 128   # the default
    with pytest.raises(ValueError, match="smaller than the training patch"):
        _set(kind, png_folder, phase="train", use_hflip=False, use_rot=False)[0]
    key = "demosaic_backend" if kind == MOSAIC else "inpaint_backend"
    with pytest.raises(ValueError, match=key):
        _set(kind, png_folder, **{key: "cv2"})
    if kind == MOSAIC:
        with pytest.raises(ValueError, match="demosaic_method"):
            _set(kind, png_folder, demosaic_method="ea")


@pytest.mark.parametrize("method", list(METHODS))
def test_mosaic_host_lq_equals_the_restatement_bit_for_bit(method, png_folder):
    ds = _set(MOSAIC, png_folder, demosaic_method=method)
    for i in range(3):
        s = ds[i]   # 40 x 48, 33 x 37 (odd both ways), 64 x 35
        want, sums, unit = R.demosaic_u8(s["gt"][None].numpy(), method)
        assert np.array_equal(s["lq"].numpy().view(np.int32), want[0].view(np.int32))
        v = s["lq"] * 255
        assert torch.equal(v, torch.round(v)) and 0 <= float(s["lq"].min()) and float(s["lq"].max()) <= 1   # on the 8-bit grid
        assert "mosaic" not in s
    # the known sample passes through: lq equals gt on the CFA sites (gt is an 8-bit image)
    s = ds[0]
    for (r, c, ch) in [(0, 0, 0), (1, 1, 2), (0, 1, 1), (1, 0, 1), (38, 46, 0), (39, 47, 2)]:
        assert s["lq"][ch, r, c] == s["gt"][ch, r, c]


def _replay_strokes(h, w, rng=random):
    l_num, l_thick = rng.randint(5, 10), rng.randint(5, 10)
    white = rng.choice(["white", "black"]) == "white"
    lines = np.zeros((10, 4), dtype=np.int32)
    for k in range(l_num):
        lines[k] = (rng.randint(0, w), rng.randint(0, h), rng.randint(0, w), rng.randint(0, h))
    return lines, [l_num, l_thick, int(white)]


def test_inpainting_draws_replay_pythons_random(png_folder):
    """the reference's order: n, thick, colour, then x1 y1 x2 y2 per stroke -- after the crop and the augmentation"""
    ds = _set(INPAINT, png_folder, inpaint_backend="device")
    random.seed(17)
    got = [ds[i % 3] for i in range(6)]
    random.seed(17)
    colours = set()
    for i, s in enumerate(got):
        lines, meta = _replay_strokes(*SIZES[NAMES[i % 3]])
        assert np.array_equal(s["inpaint_lines"].numpy(), lines) and s["inpaint_meta"].tolist() == meta
        assert 5 <= meta[0] <= 10 and 5 <= meta[1] <= 10 and not lines[meta[0]:].any()
        colours.add(meta[2])
    assert colours == {0, 1}
    # the train phase: two crop offsets, three augmentation draws, then the strokes on the 16 x 16 patch
    ds = _set(INPAINT, png_folder, phase="train", gt_size=16, use_hflip=True, use_rot=True, inpaint_backend="device")
    random.seed(5)
    got = [ds[i % 3] for i in range(6)]
    random.seed(5)
    for i, s in enumerate(got):
        h, w = SIZES[NAMES[i % 3]]
        random.randint(0, h - 16), random.randint(0, w - 16)
        random.random(), random.random(), random.random()
        lines, meta = _replay_strokes(16, 16)
        assert np.array_equal(s["inpaint_lines"].numpy(), lines) and s["inpaint_meta"].tolist() == meta
    # stroke_seed: a generator per image, the process-wide one untouched
    ds = _set(INPAINT, png_folder, inpaint_backend="device", stroke_seed=40)
    random.seed(1)
    state = random.getstate()
    s = ds[2]
    assert random.getstate() == state
    lines, meta = _replay_strokes(*SIZES["c.png"], rng=random.Random(42))
    assert np.array_equal(s["inpaint_lines"].numpy(), lines) and s["inpaint_meta"].tolist() == meta


def test_inpainting_host_lq_equals_the_restatement_bit_for_bit(png_folder):
    ds_h, ds_d = _set(INPAINT, png_folder), _set(INPAINT, png_folder, inpaint_backend="device")
    for i in range(3):
        random.seed(100 + i)
        h = ds_h[i]
        random.seed(100 + i)
        d = ds_d[i]
        assert torch.equal(h["gt"], d["gt"]) and "inpaint_meta" not in h
        want, masks = R.inpaint(d["gt"][None].numpy(), d["inpaint_lines"][None].numpy(), d["inpaint_meta"][None].numpy())
        assert np.array_equal(h["lq"].numpy().view(np.int32), want[0].view(np.int32))
        m = torch.from_numpy(masks[0])
        assert 0 < int(m.sum()) < m.numel()
        assert torch.equal(h["lq"][:, ~m], h["gt"][:, ~m])   # equal to gt off the mask
        assert bool((h["lq"][:, m] == float(d["inpaint_meta"][2])).all())


def test_device_backend_samples_and_batches(png_folder):
    from basicsr.data import build_dataloader

    ds = _set(MOSAIC, png_folder, demosaic_backend="device", demosaic_method="bilinear", center_crop=32)
    s = ds[0]
    assert sorted(s) == ["gt", "gt_path", "lq_path", "mosaic"]
    assert s["mosaic"].dtype == torch.int32 and s["mosaic"].dim() == 0 and int(s["mosaic"]) == 1
    assert int(_set(MOSAIC, png_folder, demosaic_backend="device")[0]["mosaic"]) == 0
    batch = next(iter(build_dataloader(ds, dict(phase="train", batch_size_per_gpu=2, num_worker_per_gpu=0))))
    assert tuple(batch["gt"].shape) == (2, 3, 32, 32) and batch["mosaic"].tolist() == [1, 1] and "lq" not in batch

    ds = _set(INPAINT, png_folder, inpaint_backend="device", center_crop=32)
    s = ds[0]
    assert sorted(s) == ["gt", "gt_path", "inpaint_lines", "inpaint_meta", "lq_path"]
    assert s["inpaint_lines"].dtype == s["inpaint_meta"].dtype == torch.int32
    assert tuple(s["inpaint_lines"].shape) == (10, 4) and tuple(s["inpaint_meta"].shape) == (3,)
    assert int(s["inpaint_lines"].min()) >= 0 and int(s["inpaint_lines"].max()) <= 32
    batch = next(iter(build_dataloader(ds, dict(phase="train", batch_size_per_gpu=2, num_worker_per_gpu=0))))
    assert tuple(batch["gt"].shape) == (2, 3, 32, 32) and tuple(batch["inpaint_lines"].shape) == (2, 10, 4)
    assert tuple(batch["inpaint_meta"].shape) == (2, 3) and batch["inpaint_meta"].dtype == torch.int32 and "lq" not in batch


def test_dehaze_pairs_several_hazy_files_with_one_gt(tmp_path):
    """SOTS: ``0001_0.8_0.2.jpg`` and ``0001_1_0.1.jpg`` -> ``0001.png``.  The identical-file-name reader cannot pair these."""
    import basicsr.data as D
    from basicsr.data import build_dataset
    from basicsr.utils.registry import DATASET_REGISTRY

    gt_root, lq_root = tmp_path / "gt", tmp_path / "hazy"
    gt_root.mkdir(), lq_root.mkdir()
    gts = {n: _image(f"degradecpu.haze.{n}", 20, 24) for n in ("0001", "0002")}
    for n, img in gts.items():
        _save(img, gt_root / f"{n}.png")
    hazy = {"0001_0.8_0.2.jpg": 0.7, "0001_1_0.1.jpg": 0.5, "0002_1_0.2.jpg": 0.3}
    for n, k in hazy.items():
        _save(gts[n[:4]] * k + (1 - k), lq_root / n)
    opt = dict(name="SOTS", type="PairedImageDehazeDataset", dataroot_gt=str(gt_root), dataroot_lq=str(lq_root), phase="val", suffix=".png")
    ds = build_dataset(opt)
    assert DATASET_REGISTRY.get("PairedImageDehazeDataset") is D.PairedImageDehazeDataset and isinstance(ds, D.PairedImageDehazeDataset)
    assert len(ds) == 3
    for i, n in enumerate(sorted(hazy)):
        s = ds[i]
        assert s["lq_path"] == str(lq_root / n) and s["gt_path"] == str(gt_root / f"{n[:4]}.png")   # the real lq path
        assert tuple(s["lq"].shape) == tuple(s["gt"].shape) == (3, 20, 24)
        assert torch.equal(s["gt"], D._read_rgb(str(gt_root / f"{n[:4]}.png"))) and float((s["lq"] - s["gt"]).mean()) > 0.05
    assert torch.equal(ds[0]["gt"], ds[1]["gt"]) and not torch.equal(ds[0]["lq"], ds[1]["lq"])
    assert build_dataset({k: v for k, v in opt.items() if k != "suffix"}).suffix == ".jpg"   # the reference's default
    s = build_dataset(dict(opt, center_crop=16, dataset_idx=2))[2]
    assert tuple(s["lq"].shape) == tuple(s["gt"].shape) == (3, 16, 16) and s["dataset_idx"] == 2
    random.seed(2)
    s = build_dataset(dict(opt, phase="train", gt_size=12, use_hflip=True, use_rot=True))[0]
    assert tuple(s["lq"].shape) == tuple(s["gt"].shape) == (3, 12, 12)


def test_feed_data_on_a_cpu_model_raises_the_no_cpu_fallback_error():
    """a device-backend batch reaches the kernels in feed_data -- not a KeyError for the missing lq; a batch that carries lq takes the
    path it always took"""
    from basicsr.models import build_model
    from dcpt_amd import _lib

    m = build_model(TP._opt(model_type="SRModel"))
    gt = keyed_input("degradecpu.feed", (2, 3, 16, 16))
    lines = torch.zeros((2, 10, 4), dtype=torch.int32)
    meta = torch.tensor([[5, 5, 1], [6, 7, 0]], dtype=torch.int32)
    for extra in ({"mosaic": torch.tensor([0, 0], dtype=torch.int32)}, {"inpaint_lines": lines, "inpaint_meta": meta}):
        with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
            m.feed_data({"gt": gt, **extra})
        lq = keyed_input("degradecpu.feed.lq", (2, 3, 16, 16))
        m.feed_data({"lq": lq, "gt": gt, **extra})
        assert torch.equal(m.lq, lq) and torch.equal(m.gt, gt)
    with pytest.raises(KeyError):
        m.feed_data({"gt": gt})
