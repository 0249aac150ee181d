"""CPU: the yardstick of the Gaussian-noise kernel (tests/noise_restatement.py: the Philox4x32-10 known answers and the statistics of its
normals) and the surface that needs no device: the refusals of dcpt_gauss_noise_fwd, the ``noise_backend: device`` samples of
PairedImageDenoiseDataset, ``basicsr.data.degrade_collate`` on mixed and single-kind batches, and ``feed_data`` of a CPU model.

Statistics: over N = 2^22 normals the sample mean, variance, third and fourth moment have the variances 1/N, 2/N, 15/N and 96/N and the
lag-1 correlation 1/N; each standardised figure must stay below 4 in magnitude (measured: all six keys below 2.1)."""
import os
import random

import numpy as np
import pytest
import torch

import noise_restatement as R
from dcpt_amd.keyed_init import keyed_input
from tests import test_plumbing_cpu as TP   # registers the CPU stand-in arch ``_TestConvArch``

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
STAT_KEYS = [0, 1, 0x7FFFFFFFFFFFFFFF, 0x0123456789ABCDEF, 1 << 32, (7 << 32) | 41]


@pytest.mark.parametrize("counter, key, want", KAT, ids=["zero", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{int(v):08x}" for v in R.philox4x32_10(counter, key)) == want
    # the array form gives the same words as the scalar form
    got = R.philox4x32_10([np.array([c, c]) for c in counter], key)
    assert all(v.dtype == np.uint32 and v.shape == (2,) and v[0] == v[1] for v in got)
    assert " ".join(f"{int(v[1]):08x}" for v in got) == want


@pytest.mark.parametrize("key", STAT_KEYS, ids=[hex(k) for k in STAT_KEYS])
def test_restatement_normals_have_the_moments_of_a_standard_normal(key):
    n = 1 << 22
    v = R.normals(key, n)
    assert v.dtype == np.float64 and v.shape == (n,) and np.isfinite(v).all() and float(np.abs(v).max()) < 6.8
    figs = {"mean": v.mean() * np.sqrt(n), "variance": ((v ** 2).mean() - 1.0) / np.sqrt(2.0 / n), "third": (v ** 3).mean() / np.sqrt(15.0 / n),
            "fourth": ((v ** 4).mean() - 3.0) / np.sqrt(96.0 / n), "lag-1": (v[:-1] * v[1:]).mean() * np.sqrt(n)}
    print(f"key {key:#x}: " + ", ".join(f"{k} {f:+.2f}" for k, f in figs.items()))
    for k, f in figs.items():
        assert abs(f) < 4.0, (k, f)


def test_restatement_stream_layout():
    """a prefix of a stream is the stream of the shorter length; the key's two words are its low and high half; gray noise is one plane"""
    a, b = R.normals(5, 10), R.normals(5, 103)
    assert np.array_equal(a, b[:10])
    assert not np.array_equal(R.normals(5, 8), R.normals(5 << 32, 8)) and not np.array_equal(R.normals(5, 8), R.normals(6, 8))
    assert np.array_equal(R.normals(-1, 8), R.normals((1 << 64) - 1, 8))   # an int64 key is its 64 bits
    x = np.zeros((2, 3, 5, 7), np.float32)
    t = R.gauss_noise(x, [255.0, 255.0], [9, 9], gray=[0, 1])
    assert np.array_equal(t[0].reshape(-1), R.normals(9, 105)) and np.array_equal(t[1, 0].reshape(-1), R.normals(9, 35))
    assert np.array_equal(t[1, 0], t[1, 1]) and np.array_equal(t[1, 0], t[1, 2])
    r = R.gauss_noise(x + 0.5, [25.0, 50.0], [1, 2], clip=True, rounds=True)
    assert np.array_equal(np.rint(r * 255), r * 255) and r.min() >= 0 and r.max() <= 1


def test_entry_point_refuses_bad_arguments_without_a_device():
    """every check comes before the launch: each refusal is reported, with its text, on a machine with no GPU"""
    from kernel_trace import kernel_trace

    from dcpt_amd import _lib

    lib = _lib.load()
    f = lib.dcpt_gauss_noise_fwd
    header = open(os.path.join(ROOT, "include", "dcpt_hip.h")).read()
    assert "int dcpt_gauss_noise_fwd(" in header and "dcpt_gauss_noise_fwd" in _lib.SIGNATURES
    assert "#define DCPT_NOISE_CLIP 1" in header and "#define DCPT_NOISE_ROUND8 2" in header and "#define DCPT_NOISE_ONLY 4" in header
    assert lib.dcpt_abi_version() == 16
    with kernel_trace() as t:
        for args in [(None, 16, 16, None, 16), (16, None, 16, None, 16), (16, 16, None, 16, 16), (16, 16, 16, 16, None)]:
            assert f(*args, 1, 3, 8, 8, 0, None) == 1 and b"null" in lib.dcpt_last_error(), args
        assert f(None, 16, 16, None, None, 1, 3, 8, 8, 4, None) == 1 and b"null" in lib.dcpt_last_error()   # NOISE_ONLY excuses x only
        for dims in [(0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8), (1, 3, -8, 8)]:
            assert f(16, 16, 16, None, 16, *dims, 0, None) == 1 and b"bad shape" in lib.dcpt_last_error(), dims
        for dims in [(1, 4, 1 << 16, 1 << 16), (1, 1, 1 << 17, 1 << 17), (1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1), (1, 1 << 20, 1 << 14, 1)]:
            assert f(16, 16, 16, None, 16, *dims, 0, None) == 1 and b"below 2^34" in lib.dcpt_last_error(), dims
        for flags in (8, 16, -1, 1 << 30):
            assert f(16, 16, 16, None, 16, 1, 3, 8, 8, flags, None) == 1 and b"unknown flags" in lib.dcpt_last_error(), flags
    assert t.counts == {}, t.counts


def test_ops_refuse_cpu_tensors():
    from basicsr.data import degradations as G
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    x = keyed_input("noisecpu.cpu", (2, 3, 8, 8))
    for call in (lambda: DF.gaussian_noise(x, 25, 1), lambda: G.add_gaussian_noise_pt(x, 10, key=3), lambda: G.generate_gaussian_noise_pt(x),
                 lambda: G.random_add_gaussian_noise_pt(x, (0, 10), 0.5), lambda: G.random_generate_gaussian_noise_pt(x)):
        with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
            call()
    with pytest.raises(_lib.DcptHipError):
        DF.gaussian_noise(x.numpy(), 25, 1)
    assert sorted(G.__all__) == ["add_gaussian_noise_pt", "generate_gaussian_noise_pt", "random_add_gaussian_noise_pt",
                                 "random_generate_gaussian_noise_pt"]
    for word in ("Philox", "distribution", "independent per image", "Poisson", "filter2D", "USMSharp", "numpy"):
        assert word in G.__doc__, word


# ---- the data set --------------------------------------------------------------------------------------
NAMES = ["a.png", "b.png", "c.png"]
SIZES = {"a.png": (40, 48), "b.png": (33, 37), "c.png": (64, 35)}
DENOISE = "PairedImageDenoiseDataset"


@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("noise_gt")
    for n in NAMES:
        h, w = SIZES[n]
        low = keyed_input(f"noisecpu.{n}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0].clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / n)
    return str(root)


def _set(kind, root, **over):
    from basicsr.data import build_dataset

    opt = dict(name=kind, type=kind, dataroot_gt=root, phase="val")
    opt.update(over)
    return build_dataset(opt)


def test_device_samples_keys_dtypes_and_draw_order(png_folder):
    host = _set(DENOISE, png_folder, sigma_type="choice", sigma_range=[15, 50])
    dev = _set(DENOISE, png_folder, sigma_type="choice", sigma_range=[15, 50], noise_backend="device")
    assert host.backend == "host" and dev.backend == "device"
    with pytest.raises(ValueError, match="noise_backend"):
        _set(DENOISE, png_folder, sigma_range=25, noise_backend="gpu")
    for i in range(3):
        random.seed(50 + i)
        h = host[i]
        state_h = random.getstate()
        random.seed(50 + i)
        d = dev[i]
        assert random.getstate() == state_h                       # the same draws were consumed
        random.seed(50 + i)
        sigma = random.choice([15, 50])                           # ... and the first of them is the sigma
        assert sorted(d) == ["gt", "gt_path", "lq_path", "noise_key", "noise_sigma"] and sorted(h) == ["gt", "gt_path", "lq", "lq_path"]
        assert d["noise_sigma"].dtype == torch.float32 and d["noise_sigma"].dim() == 0 and float(d["noise_sigma"]) == sigma
        assert d["noise_key"].dtype == torch.int64 and d["noise_key"].dim() == 0
        assert torch.equal(d["gt"], h["gt"]) and d["gt"].dtype == torch.float32 and d["gt"].is_contiguous()
        std = float((h["lq"] - h["gt"]).std()) * 255              # the host path's noise has that sigma
        assert abs(std - sigma) < 0.05 * sigma, (std, sigma)
    # other phases: the key is (noise_seed << 32) | index, the same on every visit
    assert [int(dev[i]["noise_key"]) for i in range(3)] == [0, 1, 2] == [int(dev[i]["noise_key"]) for i in range(3)]
    seeded = _set(DENOISE, png_folder, sigma_range=25, noise_backend="device", noise_seed=7, dataset_idx=3)
    assert [int(seeded[i]["noise_key"]) for i in range(3)] == [(7 << 32) | i for i in range(3)]
    assert seeded[0]["dataset_idx"] == 3 and float(seeded[0]["noise_sigma"]) == 25.0
    # the train phase: two crop offsets, three augmentation draws, the sigma, then 63 fresh key bits
    train = _set(DENOISE, png_folder, phase="train", gt_size=16, use_hflip=True, use_rot=True, sigma_type="random", sigma_range=[5, 45],
                 noise_backend="device")
    random.seed(8)
    got = [train[i % 3] for i in range(6)]
    random.seed(8)
    keys = []
    for i, s in enumerate(got):
        h, w = SIZES[NAMES[i % 3]]
        random.randint(0, h - 16), random.randint(0, w - 16)
        random.random(), random.random(), random.random()
        sigma = random.uniform(5, 45)
        key = random.getrandbits(63)
        assert float(s["noise_sigma"]) == float(np.float32(sigma)) and int(s["noise_key"]) == key and tuple(s["gt"].shape) == (3, 16, 16)
        keys.append(key)
    assert len(set(keys)) == 6 and all(0 <= k < (1 << 63) for k in keys)   # image 0 on its second visit draws a fresh key
    # the host path is untouched by the new option: the reference's draw, bit for bit
    random.seed(1)
    s = host[1]
    rs = np.random.RandomState(0)
    hwc = s["gt"].permute(1, 2, 0).contiguous().numpy().copy()
    random.seed(1)
    hwc += rs.normal(0, random.choice([15, 50]) / 255.0, hwc.shape)
    assert np.array_equal(s["lq"].numpy(), hwc.transpose(2, 0, 1))


# ---- degrade_collate -------------------------------------------------------------------------------------
def _five_sets(root, gt_size=16, **over):
    common = dict(phase="train", gt_size=gt_size, use_hflip=True, use_rot=True)
    specs = [(DENOISE, dict(sigma_type="choice", sigma_range=[15, 25, 50], noise_backend="device")),
             ("PairedImageJPEGCARDataset", dict(q_type="choice", q_range=[10, 40], jpeg_backend="device")),
             ("PairedImageMosaicDataset", dict(demosaic_backend="device", demosaic_method="bilinear")),
             ("PairedImageInpaintingDataset", dict(inpaint_backend="device")),
             ("PairedImageDataset", {})]
    return [_set(kind, root, **{**common, **extra, **over.get(kind, {})}) for kind, extra in specs]


KIND_OF_SET = [1, 2, 3, 4, 0]   # _five_sets order -> degrade_kind


def test_a_mixed_batch_goes_through_the_train_loader(png_folder):
    """the four device sets and one set with ``lq``, concatenated as basicsr/train.py does, batch 10 through build_dataloader: torch's
    default collate refuses such a batch (the samples carry different keys)"""
    from basicsr.data import build_dataloader, degrade_collate
    from basicsr.data.concat_dataset import ConcatDataset

    sets = _five_sets(png_folder)
    cat = ConcatDataset(sets, [1] * 5)
    assert len(cat) == 15
    random.seed(3)
    torch.manual_seed(3)
    loader = build_dataloader(cat, dict(phase="train", batch_size_per_gpu=10, num_worker_per_gpu=0))
    assert loader.collate_fn is degrade_collate
    batch = next(iter(loader))
    kind, idx = batch["degrade_kind"], batch["dataset_idx"]
    assert kind.dtype == torch.int32 and tuple(kind.shape) == (10,) and not kind.is_cuda
    assert kind.tolist() == [KIND_OF_SET[k] for k in idx.tolist()]
    count = [kind.tolist().count(k) for k in range(5)]
    assert sum(count) == 10 and sum(c > 0 for c in count) >= 3, count   # (15 samples, 3 per set, 10 drawn: at least 4 kinds in fact)
    assert tuple(batch["gt"].shape) == (10, 3, 16, 16) and len(batch["gt_path"]) == len(batch["lq_path"]) == 10 and tuple(idx.shape) == (10,)
    shapes = {"lq": (count[0], 3, 16, 16), "noise_sigma": (count[1],), "noise_key": (count[1],), "jpeg_quality": (count[2],),
              "mosaic": (count[3],), "inpaint_lines": (count[4], 10, 4), "inpaint_meta": (count[4], 3)}
    kind_of_key = {"lq": 0, "noise_sigma": 1, "noise_key": 1, "jpeg_quality": 2, "mosaic": 3, "inpaint_lines": 4, "inpaint_meta": 4}
    for key, shape in shapes.items():
        if count[kind_of_key[key]]:
            assert tuple(batch[key].shape) == shape, (key, batch[key].shape)
        else:
            assert key not in batch
    assert set(batch) == {"gt", "gt_path", "lq_path", "dataset_idx", "degrade_kind"} | {k for k in shapes if count[kind_of_key[k]]}
    assert batch["noise_sigma"].dtype == torch.float32 and batch["noise_key"].dtype == torch.int64 and batch["mosaic"].dtype == torch.int32
    assert set(batch["noise_sigma"].tolist()) <= {15.0, 25.0, 50.0} and set(batch["mosaic"].tolist()) == {1}


def test_the_row_partition_keeps_batch_order(png_folder):
    from basicsr.data import degrade_collate

    sets = _five_sets(png_folder)
    random.seed(11)
    order = [1, 0, 4, 1, 3, 2, 0, 1]          # which set each sample comes from
    samples = [dict(sets[k][i % 3], dataset_idx=k) for i, k in enumerate(order)]
    batch = degrade_collate([dict(s) for s in samples])
    assert batch["degrade_kind"].tolist() == [KIND_OF_SET[k] for k in order]
    for i, s in enumerate(samples):
        assert torch.equal(batch["gt"][i], s["gt"]) and batch["gt_path"][i] == s["gt_path"]
    rows = {kind: [s for s, k in zip(samples, order) if KIND_OF_SET[k] == kind] for kind in range(5)}
    assert torch.equal(batch["lq"], torch.stack([s["lq"] for s in rows[0]]))
    assert torch.equal(batch["noise_key"], torch.stack([s["noise_key"] for s in rows[1]]))
    assert torch.equal(batch["noise_sigma"], torch.stack([s["noise_sigma"] for s in rows[1]]))
    assert torch.equal(batch["jpeg_quality"], torch.stack([s["jpeg_quality"] for s in rows[2]]))
    assert torch.equal(batch["mosaic"], torch.stack([s["mosaic"] for s in rows[3]]))
    assert torch.equal(batch["inpaint_lines"], torch.stack([s["inpaint_lines"] for s in rows[4]]))
    assert torch.equal(batch["inpaint_meta"], torch.stack([s["inpaint_meta"] for s in rows[4]]))
    with pytest.raises(ValueError, match="exactly one of"):
        degrade_collate([samples[0], {k: v for k, v in samples[1].items() if not k.startswith("noise_")}])
    with pytest.raises(ValueError, match="exactly one of"):
        degrade_collate([samples[0], dict(samples[1], mosaic=torch.tensor(0, dtype=torch.int32))])


def test_single_kind_batches_equal_default_collate(png_folder):
    """nothing that works today changes: key by key, bit for bit"""
    from torch.utils.data import default_collate

    from basicsr.data import degrade_collate

    for ds in _five_sets(png_folder):
        random.seed(21)
        samples = [ds[i] for i in range(3)]
        got, want = degrade_collate([dict(s) for s in samples]), default_collate([dict(s) for s in samples])
        assert list(got) == list(want) and "degrade_kind" not in got
        for k in want:
            if torch.is_tensor(want[k]):
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape
                assert torch.equal(got[k].contiguous().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k
            else:
                assert got[k] == want[k], k


def test_gt_sizes_that_differ_are_refused(png_folder):
    from basicsr.data import degrade_collate

    sets = _five_sets(png_folder, **{DENOISE: dict(gt_size=24)})
    random.seed(2)
    with pytest.raises(ValueError, match="gt_size"):
        degrade_collate([sets[0][0], sets[1][0], sets[2][0]])


def test_feed_data_on_a_cpu_model_raises_the_no_cpu_fallback_error(png_folder):
    """a noise batch and a mixed batch reach the kernels in feed_data -- not a KeyError for the missing lq"""
    from basicsr.data import degrade_collate
    from basicsr.models import build_model
    from dcpt_amd import _lib

    m = build_model(TP._opt(model_type="SRModel"))
    gt = keyed_input("noisecpu.feed", (2, 3, 16, 16))
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        m.feed_data({"gt": gt, "noise_sigma": torch.tensor([15.0, 25.0]), "noise_key": torch.tensor([1, 2])})
    sets = _five_sets(png_folder)
    random.seed(4)
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        m.feed_data(degrade_collate([sets[0][0], sets[3][1]]))
    batch = degrade_collate([sets[4][0], sets[4][1]])          # a batch that carries lq takes the path it always took
    m.feed_data(batch)
    assert torch.equal(m.lq, batch["lq"]) and torch.equal(m.gt, batch["gt"])
    with pytest.raises(ValueError, match="degrade_kind"):
        m.feed_data({"gt": gt, "degrade_kind": torch.tensor([0, 7], dtype=torch.int32), "lq": gt})


def test_shipped_option_files_parse_and_name_device_backends():
    import yaml

    with open(os.path.join(ROOT, "options", "all_in_one", "train", "train_DCPT_NAFNet_4d_device.yml")) as f:
        opt = yaml.safe_load(f)
    train = [v for k, v in opt["datasets"].items() if k.startswith("train")]
    assert [d["type"] for d in train] == [DENOISE, "PairedImageJPEGCARDataset", "PairedImageMosaicDataset", "PairedImageInpaintingDataset"]
    assert [d.get("noise_backend") or d.get("jpeg_backend") or d.get("demosaic_backend") or d.get("inpaint_backend") for d in train] == ["device"] * 4
    assert len({d["dataroot_gt"] for d in train}) == 1 and len({d["gt_size"] for d in train}) == 1 and all(d["allow_synthetic"] for d in train)
    assert opt["network_dc"]["num_classes"] == 4 and opt["model_type"] == "DCPTModel"
    for name in ("train_NAFNet_denoise.yml", "test_NAFNet_denoise.yml"):
        with open(os.path.join(ROOT, "options", "denoise", name)) as f:
            sets = yaml.safe_load(f)["datasets"]
        assert all(d["type"] == DENOISE for d in sets.values()) and any(d.get("noise_backend") == "device" for d in sets.values())
