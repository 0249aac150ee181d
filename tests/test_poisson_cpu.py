"""CPU: the yardstick of the Poisson-noise kernels (tests/poisson_restatement.py: its sampler against the exact Poisson law, the termination
of the search, its level count against the reference's ``torch.unique`` expression) and the surface that needs no device: the refusals
of dcpt_poisson_noise_fwd and its workspace query, the ops on CPU tensors, the ``noise_type: poisson`` samples of
PairedImageDenoiseDataset and ``degrade_collate`` on them.

Kolmogorov bound: over N = 4096 draws the largest distance D between the empirical and the exact CDF exceeds eps with probability at most
2 exp(-2 N eps^2) (Dvoretzky-Kiefer-Wolfowitz; it holds for discrete laws too).  eps = 0.03 gives 1.3e-3 per rate.  The draws are
deterministic: with the key below the five rates give D = 0, 0.0067, 0.0077, 0.0097 and 0.0080, a margin of 3x or more."""
import math
import os
import random

import numpy as np
import pytest
import torch

import poisson_restatement as P
from dcpt_amd.keyed_init import keyed_input
from poisson_cases import CASES, PALETTE_LEVELS, case_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAW_KEY, LAW_N, LAW_EPS = 0x5EED0000BEEF, 4096, 0.03
DENOISE = "PairedImageDenoiseDataset"
NAMES = ["a.png", "b.png", "c.png"]
SIZES = {"a.png": (40, 48), "b.png": (33, 37), "c.png": (64, 35)}


@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("poisson_gt")
    for n in NAMES:
        h, w = SIZES[n]
        low = keyed_input(f"poissoncpu.{n}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0].clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / n)
    return str(root)


def _set(kind, root, **over):
    from basicsr.data import build_dataset

    opt = dict(name=kind, type=kind, dataroot_gt=root, phase="val")
    opt.update(over)
    return build_dataset(opt)


def _cdf(lam, kmax):
    if lam == 0:
        return np.ones(kmax + 1)
    return np.cumsum([math.exp(k * math.log(lam) - lam - math.lgamma(k + 1)) for k in range(kmax + 1)])


@pytest.mark.parametrize("lam", [0.0, 0.5, 3.0, 40.0, 256.0])
def test_restatement_sampler_follows_the_poisson_law(lam):
    k = P.draws(LAW_KEY, lam, LAW_N)
    assert k.shape == (LAW_N,) and k.min() >= 0
    kmax = int(k.max())
    emp = np.cumsum(np.bincount(k, minlength=kmax + 1)) / LAW_N
    D = float(np.abs(emp - _cdf(lam, kmax)).max())
    print(f"lambda {lam}: D = {D:.4f} over {LAW_N} draws (bound {LAW_EPS}); mean {k.mean():.3f}, variance {k.var():.3f}, largest k {kmax}")
    assert D < LAW_EPS
    if lam == 0:
        assert kmax == 0
    # the table look-up is the loop of the header: the same k, draw by draw
    u = P.uniforms(LAW_KEY, 64)
    assert [P.search_literal(lam, v) for v in u] == k[:64].tolist()


def test_the_search_ends_long_before_its_cap():
    """lambda = 256, the largest rate: over 2^20 counters (2^22 draws) the largest k is far below 1023, and the partial sums pass the
    largest possible u = 1 - 2^-33 before the cap -- for every rate the kernels can meet (256 levels x the 9 values of vals)"""
    k = P.draws(1, 256.0, 1 << 22)
    print(f"lambda 256: largest k over 2^22 draws {int(k.max())}, smallest {int(k.min())}")
    assert 150 < int(k.min()) and int(k.max()) < 400
    umax = 1.0 - 2.0 ** -33
    assert float(P.uniforms(0, 4).max()) <= umax and (0xFFFFFFFF + 0.5) * 2.0 ** -32 == umax
    lam = np.array([[l * (1 << e) / 255.0 for l in range(256)] for e in range(9)])
    S = P.cumulative(lam)
    first = (S >= umax).argmax(-1)
    assert bool((S[..., -1] >= umax).all())
    print(f"the sums pass 1 - 2^-33 at k <= {int(first.max())} for every (level, vals)")
    assert int(first.max()) < 400
    assert bool((np.diff(S, axis=-1) >= 0).all())   # never decreasing: what the table look-up of the restatement rests on


def _reference_vals(img):
    """``vals`` as the reference computes it (generate_poisson_noise_pt): fp32 rounding, torch.unique, 2 ** ceil(log2)"""
    q = torch.clamp((img * 255.0).round(), 0, 255) / 255.0
    return int(2 ** np.ceil(np.log2(len(torch.unique(q)))))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_vals_equal_the_reference_expression(name):
    x, scale, key, gray = case_args(name)
    r = P.poisson_noise(x.numpy(), scale.numpy(), key.tolist(), None if gray is None else gray.tolist())
    for b in range(x.shape[0]):
        img = x[b:b + 1]
        if gray is not None and int(gray[b]) and x.shape[1] == 3:
            img = 0.2989 * img[:, 0:1] + 0.587 * img[:, 1:2] + 0.114 * img[:, 2:3]   # (torchvision's rgb_to_grayscale, fp32)
        want = _reference_vals(img)
        assert int(r.vals[b]) == want == 2 ** math.ceil(math.log2(int(r.U[b]))), (b, int(r.U[b]), int(r.vals[b]), want)
    print(f"{name}: U {r.U.tolist()} vals {r.vals.tolist()}; largest k {int(r.k.max())}; excluded {int(r.near_level.sum())} near a level "
          f"boundary, {int(r.near_u.sum())} near a partial sum")
    assert int(r.near_level.sum()) == 0 and int(r.near_u.sum()) == 0   # the cases exclude NOTHING
    if name == "palettes":
        assert r.U.tolist() == list(PALETTE_LEVELS) and r.vals.tolist() == [16, 32, 256, 256]
    if name == "zeros":
        assert r.U.tolist() == [1] and r.vals.tolist() == [1] and int(r.k.max()) == 0 and float(np.abs(r.T).max()) == 0.0
    if name == "2x3x64x65":
        assert r.U.tolist() == [256, 256]
    if name == "1x1x1x1":
        assert r.vals.tolist() == [1]


def test_restatement_layout():
    """gray noise is one plane shared by the channels and reads u per PIXEL; colour noise reads u per element; scale and flags"""
    x, scale, key, gray = case_args("2x3x5x7")
    r = P.poisson_noise(x.numpy(), [1.0, 1.0], [9, 9], [0, 1], noise_only=True)
    assert np.array_equal(r.T[1, 0], r.T[1, 1]) and np.array_equal(r.T[1, 0], r.T[1, 2]) and not np.array_equal(r.T[0, 0], r.T[0, 1])
    lev = P.level(x[0].double().numpy())
    assert np.array_equal(r.T[0], r.k[0] / float(r.vals[0]) - lev / 255.0)
    half = P.poisson_noise(x.numpy(), [0.5, 0.5], [9, 9], [0, 1], noise_only=True)
    assert np.array_equal(half.T, 0.5 * r.T) and np.array_equal(half.k, r.k)
    c = P.poisson_noise(x.numpy(), [1.0, 1.0], [9, 9], [0, 1], clip=True, rounds=True)
    assert np.array_equal(np.rint(c.T * 255), c.T * 255) and c.T.min() >= 0 and c.T.max() <= 1
    assert P.level(np.array([np.nan, -1.0, 2.0, 0.5 / 255, 1.5 / 255, np.inf])).tolist() == [0, 0, 255, 0, 2, 255]


# ---- the entry point without a device ---------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_without_a_device():
    from kernel_trace import kernel_trace

    from dcpt_amd import _lib

    lib = _lib.load()
    f = lib.dcpt_poisson_noise_fwd
    header = open(os.path.join(ROOT, "include", "dcpt_hip.h")).read()
    assert "int dcpt_poisson_noise_fwd(" in header and "size_t dcpt_poisson_noise_ws_bytes(" in header
    assert "dcpt_poisson_noise_fwd" in _lib.SIGNATURES and "dcpt_poisson_noise_ws_bytes" in _lib.SIGNATURES
    assert lib.dcpt_abi_version() == 16
    big = 1 << 30
    with kernel_trace() as t:
        for args in [(None, 16, 16, None, 16, 16), (16, None, 16, None, 16, 16), (16, 16, None, 16, 16, 16), (16, 16, 16, 16, None, 16),
                     (16, 16, 16, None, 16, None)]:
            assert f(*args, big, 1, 3, 8, 8, 0, None) == 1 and b"null" in lib.dcpt_last_error(), args
        assert f(None, 16, 16, None, 16, 16, big, 1, 3, 8, 8, 4, None) == 1 and b"null" in lib.dcpt_last_error()   # NOISE_ONLY still reads x
        for dims in [(0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8), (1, 3, -8, 8)]:
            assert f(16, 16, 16, None, 16, 16, big, *dims, 0, None) == 1 and b"bad shape" in lib.dcpt_last_error(), dims
        for dims in [(1, 4, 1 << 16, 1 << 16), (1, 1, 1 << 17, 1 << 17), (1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1), (1, 1 << 20, 1 << 14, 1)]:
            assert f(16, 16, 16, None, 16, 16, big, *dims, 0, None) == 1 and b"below 2^34" in lib.dcpt_last_error(), dims
        assert f(16, 16, 16, None, 16, 16, big, 1 << 20, 1, 1 << 11, 1 << 11, 0, None) == 1 and b"2^40" in lib.dcpt_last_error()
        for flags in (8, 16, -1, 1 << 30):
            assert f(16, 16, 16, None, 16, 16, big, 1, 3, 8, 8, flags, None) == 1 and b"unknown flags" in lib.dcpt_last_error(), flags
        for C in (2, 4, 5):
            assert f(16, 16, 16, 16, 16, 16, big, 1, C, 8, 8, 0, None) == 1 and b"C = 1 or 3" in lib.dcpt_last_error(), C
        need = lib.dcpt_poisson_noise_ws_bytes(2, 3, 8, 8)
        for have in (0, 8, need - 1):
            assert f(16, 16, 16, None, 16, 16, have, 2, 3, 8, 8, 0, None) == 2 and b"workspace too small" in lib.dcpt_last_error(), have
    assert t.counts == {}, t.counts


def test_workspace_query_needs_no_device():
    from dcpt_amd import _lib

    q = _lib.load().dcpt_poisson_noise_ws_bytes
    assert q(0, 3, 8, 8) == 0 and q(1, 3, -1, 8) == 0 and q(1, 4, 1 << 16, 1 << 16) == 0
    small, one_more, many = q(1, 1, 1, 1), q(1, 3, 64, 65), q(32, 3, 256, 256)
    assert small >= 4 + 32 and small % 256 == 0                       # vals[1] and one 256-bit mask
    assert one_more >= 4 + 4 * 32 and many >= 32 * 4 + 32 * 32 * 32    # 4 chunks of 4096 elements; the chunk count stops at 32
    assert q(32, 3, 2048, 2048) == many                               # ... however large the image
    assert q(64, 3, 256, 256) > many


def test_ops_refuse_cpu_tensors():
    from basicsr.data import degradations as G
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    x = keyed_input("poissoncpu.cpu", (2, 3, 8, 8))
    for call in (lambda: DF.poisson_noise(x, 1.0, 1), lambda: G.add_poisson_noise_pt(x, 1.0, key=3), lambda: G.generate_poisson_noise_pt(x),
                 lambda: G.random_add_poisson_noise_pt(x, (0, 1.0), 0.5), lambda: G.random_generate_poisson_noise_pt(x)):
        with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
            call()
    with pytest.raises(_lib.DcptHipError):
        DF.poisson_noise(x.numpy(), 1.0, 1)
    import inspect

    for name, ref in (("generate_poisson_noise_pt", ["img", "scale", "gray_noise"]), ("add_poisson_noise_pt", ["img", "scale", "clip", "rounds", "gray_noise"]),
                      ("random_generate_poisson_noise_pt", ["img", "scale_range", "gray_prob"]),
                      ("random_add_poisson_noise_pt", ["img", "scale_range", "gray_prob", "clip", "rounds"])):
        assert list(inspect.signature(getattr(G, name)).parameters) == ref + ["key"], name
    d = {k: p.default for k, p in inspect.signature(G.add_poisson_noise_pt).parameters.items()}
    assert d["scale"] == 1.0 and d["clip"] is True and d["rounds"] is False and d["gray_noise"] == 0 and d["key"] is None
    for word in ("Poisson", "distribution", "fp64", "2^-32", "1 or 3 channels"):
        assert word in G.__doc__, word


# ---- the data set -----------------------------------------------------------------------------------------
def test_poisson_samples_of_the_denoise_set(png_folder):
    with pytest.raises(ValueError, match="noise_backend: device"):
        _set(DENOISE, png_folder, noise_type="poisson")
    with pytest.raises(ValueError, match="noise_backend: device"):
        _set(DENOISE, png_folder, noise_type="poisson", noise_backend="host")
    with pytest.raises(ValueError, match="noise_type"):
        _set(DENOISE, png_folder, sigma_range=25, noise_type="speckle")
    val = _set(DENOISE, png_folder, noise_type="poisson", noise_backend="device", poisson_scale=0.5, noise_seed=7)
    for i in range(3):
        s = val[i]
        assert sorted(s) == ["gt", "gt_path", "lq_path", "noise_key", "poisson_gray", "poisson_scale"]
        assert s["poisson_scale"].dtype == torch.float32 and s["poisson_scale"].dim() == 0 and float(s["poisson_scale"]) == 0.5
        assert s["poisson_gray"].dtype == torch.int32 and int(s["poisson_gray"]) == 0
        assert s["noise_key"].dtype == torch.int64 and int(s["noise_key"]) == (7 << 32) | i == int(val[i]["noise_key"])   # the same on every visit
        assert s["gt"].dtype == torch.float32 and s["gt"].is_contiguous()
    # the train phase: two crop offsets, three augmentation draws, the scale, the gray decision, then 63 fresh key bits
    train = _set(DENOISE, png_folder, phase="train", gt_size=16, use_hflip=True, use_rot=True, noise_type="poisson", noise_backend="device",
                 poisson_scale=[0.05, 3.0], gray_prob=0.4)
    random.seed(8)
    got = [train[i % 3] for i in range(6)]
    random.seed(8)
    grays = []
    for i, s in enumerate(got):
        h, w = SIZES[NAMES[i % 3]]
        random.randint(0, h - 16), random.randint(0, w - 16)
        random.random(), random.random(), random.random()
        scale = random.uniform(0.05, 3.0)
        gray = random.random() < 0.4
        key = random.getrandbits(63)
        assert float(s["poisson_scale"]) == float(np.float32(scale)) and int(s["poisson_gray"]) == int(gray) and int(s["noise_key"]) == key
        assert tuple(s["gt"].shape) == (3, 16, 16)
        grays.append(gray)
    assert 0 < sum(grays) < 6
    # the default noise type is untouched by the new option
    assert sorted(_set(DENOISE, png_folder, sigma_range=25, noise_backend="device")[0]) == ["gt", "gt_path", "lq_path", "noise_key", "noise_sigma"]


def test_degrade_collate_takes_poisson_batches_and_refuses_them_next_to_another_kind(png_folder):
    from torch.utils.data import default_collate

    from basicsr.data import degrade_collate

    pois = _set(DENOISE, png_folder, phase="train", gt_size=16, noise_type="poisson", noise_backend="device", poisson_scale=1.0)
    gaus = _set(DENOISE, png_folder, phase="train", gt_size=16, sigma_range=25, noise_backend="device")
    random.seed(3)
    samples = [pois[i] for i in range(3)]
    got, want = degrade_collate([dict(s) for s in samples]), default_collate([dict(s) for s in samples])
    assert list(got) == list(want) and "degrade_kind" not in got and tuple(got["poisson_scale"].shape) == (3,)
    assert torch.equal(got["noise_key"], want["noise_key"]) and torch.equal(got["poisson_gray"], want["poisson_gray"])
    with pytest.raises(ValueError, match="exactly one of"):
        degrade_collate([pois[0], gaus[1]])


def test_the_shipped_poisson_option_file_parses():
    import yaml

    with open(os.path.join(ROOT, "options", "denoise", "train_NAFNet_denoise_poisson.yml")) as f:
        sets = yaml.safe_load(f)["datasets"]
    assert all(d["type"] == DENOISE and d["noise_type"] == "poisson" and d["noise_backend"] == "device" for d in sets.values())
    assert any(isinstance(d["poisson_scale"], list) for d in sets.values())
