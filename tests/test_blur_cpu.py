"""No GPU: the blur-kernel generators of basicsr.data.degradations against the reference's kernels (tests/golden/blur_kernels.npz), the
float64 restatement of the blur (tests/blur_restatement.py) against the reference's ``filter2D`` / ``USMSharp`` outputs
(tests/golden/filter2d.npz), ``filter2d_host`` against the restatement, PairedImageBlurDataset, ``degrade_collate`` with a blur set, and
the refusals of the entry point and of the Python op.  Fixtures: tools/make_golden_blur.py.

Bounds:
* kernels: ``|k - k_ref| <= 1e-12`` per entry.  Entries are at most 1 and sum to 1; each is an ``exp``, ``pow`` or reciprocal of a quadratic
  form and one normalisation over at most 441 terms: a few hundred float64 roundings, about 1e-13.  (The tool printed 0 for every case.)
* restatement against the reference's fp32 ``filter2D``: ``K^2 2^-24`` per element, the worst-case bound of an fp32 dot product of K^2 terms
  with inputs in [0, 1] and non-negative taps summing to 1 (every partial sum is at most 1, each of the K^2 additions and products rounds
  by at most 2^-24 relative).  The restatement's own error (float64) is eight orders below it.
* USM: the output is ``soft * sharp + (1 - soft) * img`` with ``sharp = clip(img + w (img - blur))``, all in [0, 1] and w = 0.5: an error d of
  each blur moves it by at most ``|sharp - img| d + soft w d <= 1.5 d``, and the five element-wise fp32 roundings add less than 1e-6; so
  ``2 K^2 2^-24`` with the blur bound d = K^2 2^-24 applied to both blurs.  No pixel of the fixture lies within 1e-3 of the mask's step
  (the tool asserts it), so the step mask itself is the same on both sides.

Every bounded case prints its figure before it asserts."""
import math
import os
import random

import numpy as np
import pytest
import torch

import blur_restatement as R
from dcpt_amd.keyed_init import keyed_input

KINDS = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")
FILTER_CASES = {"per_image": 21, "shared": 5, "tiny": 7}


@pytest.fixture(scope="module")
def kernels(golden_dir):
    return np.load(os.path.join(golden_dir, "blur_kernels.npz"))


@pytest.fixture(scope="module")
def vectors(golden_dir):
    return np.load(os.path.join(golden_dir, "filter2d.npz"))


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _mixed_args(z):
    return {k: tuple(z[f"mixed.{k}"].tolist()) for k in ("sigma_x_range", "sigma_y_range", "rotation_range", "betag_range", "betap_range")}


def _close(k, ref, what):
    d = float(np.abs(k - ref).max())
    print(f"{what}: max |k - k_ref| {d:.3e}, |sum - 1| {abs(float(k.sum()) - 1):.3e}")
    assert k.dtype == np.float64 and k.shape == ref.shape and d <= 1e-12 and abs(float(k.sum()) - 1) <= 1e-12


# ---- the generators -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [7, 21])
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_kernels_equal_the_reference_under_its_seed(kind, K, kernels):
    from basicsr.data import degradations as G

    seed, args = int(kernels[f"mixed.{kind}.{K}.seed"]), _mixed_args(kernels)
    _seed(seed)
    k = G.random_mixed_kernels([kind], [1.0], K, noise_range=None, **args)
    _close(k, kernels[f"mixed.{kind}.{K}.kernel"], f"random_mixed_kernels {kind} K={K}")
    # rng= in place of the two modules: the same draws in the same order
    _seed(0)
    k2 = G.random_mixed_kernels([kind], [1.0], K, noise_range=None, rng=(random.Random(seed), np.random.RandomState(seed)), **args)
    assert np.array_equal(k2, k)


@pytest.mark.parametrize("tag", ["gauss_noise", "gauss_noise_iso", "ggauss_noise", "ggauss_noise_iso"])
def test_noisy_kernels_equal_the_reference_under_its_seed(tag, kernels):
    from basicsr.data import degradations as G

    seed, K, iso, args = int(kernels[f"{tag}.seed"]), int(kernels[f"{tag}.K"]), bool(kernels[f"{tag}.isotropic"]), _mixed_args(kernels)
    noise = tuple(kernels["noise_range"].tolist())
    a = (K, args["sigma_x_range"], args["sigma_y_range"], args["rotation_range"])
    if tag.startswith("gg"):
        def fn(**kw):
            return G.random_bivariate_generalized_Gaussian(*a, args["betag_range"], noise_range=noise, isotropic=iso, **kw)
    else:
        def fn(**kw):
            return G.random_bivariate_Gaussian(*a, noise_range=noise, isotropic=iso, **kw)
    _seed(seed)
    k = fn()
    _close(k, kernels[f"{tag}.kernel"], tag)
    assert np.array_equal(fn(rng=(random.Random(seed), np.random.RandomState(seed))), k)
    _seed(seed)
    plain = (G.random_bivariate_generalized_Gaussian(*a, args["betag_range"], isotropic=iso) if tag.startswith("gg")
             else G.random_bivariate_Gaussian(*a, isotropic=iso))
    assert not np.array_equal(plain, k)   # the noise is there


def test_circular_lowpass_kernels_equal_the_reference(kernels):
    from basicsr.data import degradations as G

    for i in range(3):
        cutoff, K, pad_to = kernels[f"sinc.{i}.args"].tolist()
        k = G.circular_lowpass_kernel(cutoff, int(K), int(pad_to))
        _close(k, kernels[f"sinc.{i}.kernel"], f"circular_lowpass_kernel {cutoff:.4f} {int(K)} pad_to={int(pad_to)}")
    assert k.shape == (21, 21) and not k[:4].any() and not k[:, -4:].any()   # the last case is padded from 13 to 21


def test_deterministic_kernels_and_helpers():
    from basicsr.data import degradations as G

    xy, xx, yy = G.mesh_grid(5)
    assert xy.shape == (5, 5, 2) and xx[0].tolist() == [-2, -1, 0, 1, 2] and yy[:, 0].tolist() == [-2, -1, 0, 1, 2]
    assert np.array_equal(xy[..., 0], xx) and np.array_equal(xy[..., 1], yy)
    s = G.sigma_matrix2(2.0, 1.0, math.pi / 2)
    assert np.allclose(s, [[1, 0], [0, 4]], atol=1e-12)
    g = G.bivariate_Gaussian(9, 1.5, 3.0, 0.3, isotropic=False)
    assert np.array_equal(G.bivariate_generalized_Gaussian(9, 1.5, 3.0, 0.3, 1.0, isotropic=False), g)   # beta = 1 is the Gaussian
    assert abs(g.sum() - 1) <= 1e-12 and np.allclose(g, g[::-1, ::-1], atol=1e-15) and not np.allclose(g, g[::-1])
    iso = G.bivariate_Gaussian(9, 1.5, 99.0, 1.0)
    assert np.allclose(iso, iso.T, atol=1e-16) and np.allclose(iso, iso[::-1], atol=1e-16)
    one_d = np.exp(-np.arange(-4, 5.0) ** 2 / (2 * 1.5 ** 2))
    assert np.abs(iso - np.outer(one_d, one_d) / one_d.sum() ** 2).max() <= 1e-15
    p = G.bivariate_plateau(7, 2.0, 2.0, 0.0, 2.0)
    assert abs(p.sum() - 1) <= 1e-12 and p[3, 3] == p.max() and abs(p[3, 3] / p[3, 5] - 2.0) <= 1e-12   # 1 / (1 + ((4 / 4)^2)) = 1 / 2
    c = G.cdf2(np.eye(2), xy)
    assert c.shape == (5, 5) and abs(c[2, 2] - 0.25) <= 1e-4 and c[4, 4] > 0.9 > 0.1 > c[0, 0]   # (scipy integrates numerically)
    with pytest.raises(AssertionError):
        G.random_bivariate_Gaussian(8, (0.6, 5), (0.6, 5), (-1, 1))
    with pytest.raises(ValueError, match="unknown kernel type"):
        G.random_mixed_kernels(["skew"], [1.0])


# ---- the restatement and the host form ------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(FILTER_CASES))
def test_restatement_against_the_reference_filter2d(tag, vectors):
    x, kern, y = vectors[f"{tag}.x"], vectors[f"{tag}.kernel"], vectors[f"{tag}.y"]
    K = FILTER_CASES[tag]
    assert kern.shape[-1] == K and y.dtype == np.float32 and y.shape == x.shape and (kern >= 0).all() and 0 <= x.min() and x.max() <= 1
    d = float(np.abs(R.filter2d(x, kern) - y).max())
    print(f"restatement against the reference's filter2D, {tag} {x.shape} K={K}: max |d| {d:.3e}, bound {K * K * 2.0 ** -24:.3e}")
    assert d <= K * K * 2.0 ** -24


def test_restatement_against_the_reference_usm(vectors):
    x, y, kern = vectors["usm.x"], vectors["usm.y"], vectors["usm.kernel"]
    radius, weight, threshold = vectors["usm.args"].tolist()
    out = R.usm_sharp(torch.from_numpy(x), torch.from_numpy(kern), weight, threshold).numpy()
    d = float(np.abs(out.astype(np.float64) - y).max())
    bound = 2 * radius * radius * 2.0 ** -24
    print(f"restated USMSharp.forward against the reference's, {x.shape} radius {int(radius)}: max |d| {d:.3e}, bound {bound:.3e}")
    assert kern.shape == (1, 11, 11) and d <= bound and float(np.abs(y - x).max()) > 0.01
    # the fixture's kernel is this project's Gaussian
    from basicsr.utils import USMSharp

    assert torch.equal(USMSharp(int(radius)).kernel, torch.from_numpy(kern))


@pytest.mark.parametrize("tag", list(FILTER_CASES))
def test_filter2d_host_equals_the_restatement_bit_for_bit(tag, vectors):
    from basicsr.data import filter2d_host

    x, kern = vectors[f"{tag}.x"], vectors[f"{tag}.kernel"]
    want = R.filter2d_f32(x, kern)
    for b in range(x.shape[0]):
        k = kern[b if kern.shape[0] > 1 else 0]
        got = filter2d_host(torch.from_numpy(x[b]), torch.from_numpy(k))
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want[b].view(torch.int32)), (tag, b)
        assert np.array_equal(filter2d_host(x[b], k.astype(np.float64)).view(np.int32), want[b].numpy().view(np.int32))   # arrays too
    for bad in (np.ones((4, 4), np.float32), np.ones((3, 5), np.float32), np.ones((9, 9), np.float32), np.ones((53, 53), np.float32)):
        with pytest.raises(ValueError):
            filter2d_host(x[0][:, :4, :4], bad)


def test_usm_sharp_numpy_form(vectors):
    """the HWC numpy form on filter2d_host: the same steps as the module's forward around the same blur"""
    from basicsr.utils import usm_sharp

    x = vectors["usm.x"][0]
    out = usm_sharp(np.ascontiguousarray(x.transpose(1, 2, 0)), weight=0.5, radius=10, threshold=10)   # (10 is made odd: 11)
    want = R.usm_sharp(torch.from_numpy(x[None]), torch.from_numpy(vectors["usm.kernel"]), 0.5, 10)[0].numpy().transpose(1, 2, 0)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), np.ascontiguousarray(want).view(np.int32))


def test_usmsharp_module_and_filter2D_surface():
    from basicsr.utils import USMSharp, filter2D
    from dcpt_amd import _lib

    m = USMSharp()
    sd = m.state_dict()
    assert list(sd) == ["kernel"] and tuple(sd["kernel"].shape) == (1, 51, 51) and sd["kernel"].dtype == torch.float32 and m.radius == 51
    assert abs(float(sd["kernel"].double().sum()) - 1) < 1e-6 and torch.equal(sd["kernel"][0], sd["kernel"][0].T)
    sigma = 0.3 * ((51 - 1) * 0.5 - 1) + 0.8
    one_d = np.exp(-(np.arange(51) - 25.0) ** 2 / (2 * sigma ** 2))
    assert np.abs(sd["kernel"][0].numpy() - np.outer(one_d, one_d) / one_d.sum() ** 2).max() <= 2.0 ** -24
    assert tuple(USMSharp(12, 1.5).kernel.shape) == (1, 13, 13) and tuple(USMSharp(6, 1.0).kernel.shape) == (1, 7, 7)
    for radius, sigma in ((7, 0), (6, 0), (3, -1.0), (53, 0), (52, 2.0)):
        with pytest.raises(ValueError):
            USMSharp(radius, sigma)
    x = keyed_input("blurcpu.surface", (1, 3, 8, 8))
    with pytest.raises(ValueError, match="Wrong kernel size"):
        filter2D(x, torch.ones(1, 4, 4))
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        filter2D(x, torch.ones(1, 3, 3))
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        m(keyed_input("blurcpu.usm", (1, 3, 30, 30)))


# ---- the entry point and the Python op --------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_without_a_device():
    """every check comes before the launch: each refusal is reported, with its text, on a machine with no GPU"""
    from kernel_trace import kernel_trace

    from dcpt_amd import _lib

    lib = _lib.load()
    f = lib.dcpt_filter2d_fwd
    X, KN, Y = 1 << 20, 1 << 12, 1 << 24   # addresses that are never dereferenced
    with kernel_trace() as t:
        for args in [(None, KN, Y), (X, None, Y), (X, KN, None)]:
            assert f(*args, 1, 3, 8, 8, 3, 1, None) == 1 and b"null" in lib.dcpt_last_error()
        for dims in [(0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8)]:
            assert f(X, KN, Y, *dims, 3, 1, None) == 1 and b"bad shape" in lib.dcpt_last_error(), dims
        for K in (0, -1, 2, 4, 50, 52, 53):
            assert f(X, KN, Y, 1, 3, 64, 64, K, 1, None) == 1 and b"K must be odd and lie in 1..51" in lib.dcpt_last_error(), K
        for H, W, K in [(1, 8, 3), (8, 1, 3), (10, 64, 21), (64, 10, 21), (25, 25, 51)]:
            assert f(X, KN, Y, 1, 3, H, W, K, 0, None) == 1 and b"reflect padding" in lib.dcpt_last_error(), (H, W, K)
        n = 2 * 3 * 8 * 8 * 4
        for x, y in [(X, X), (X, X + 4), (X, X + n - 4), (X + n - 4, X)]:
            assert f(x, KN, y, 2, 3, 8, 8, 3, 1, None) == 1 and b"overlaps" in lib.dcpt_last_error(), (x, y)
        assert f(X, KN, Y, 1 << 20, 1 << 11, 8, 8, 3, 1, None) == 1 and b"tiles" in lib.dcpt_last_error()
    assert t.counts == {}, t.counts


def test_header_and_ctypes_table_carry_the_name():
    from dcpt_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dcpt_hip.h")).read()
    assert "int dcpt_filter2d_fwd(" in header and "dcpt_filter2d_fwd" in _lib.SIGNATURES
    assert "acc = fma((double)kern[b][dy][dx]" in header
    assert _lib.load().dcpt_abi_version() == 16 == _lib.ABI_VERSION


def test_the_op_refuses_cpu_tensors_and_bad_shapes():
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    x = keyed_input("blurcpu.cpu", (2, 3, 8, 8))
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        DF.filter2d(x, torch.ones(2, 3, 3))
    with pytest.raises(_lib.DcptHipError):
        DF.filter2d(x.numpy(), torch.ones(2, 3, 3))
    with pytest.raises(_lib.DcptHipError):
        DF.filter2d(x.double(), torch.ones(2, 3, 3))


# ---- the data set ------------------------------------------------------------------------------------------
NAMES = ["a.png", "b.png", "c.png"]
SIZES = {"a.png": (40, 48), "b.png": (33, 37), "c.png": (64, 35)}
BLUR = "PairedImageBlurDataset"


@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("blur_gt")
    for n in NAMES:
        h, w = SIZES[n]
        low = keyed_input(f"blurcpu.{n}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
        img = (img + keyed_input(f"blurcpu.{n}.n", (3, h, w), lo=-0.05, hi=0.05)).clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / n)
    return str(root)


def _set(kind, root, **over):
    from basicsr.data import build_dataset

    opt = dict(name=kind, type=kind, dataroot_gt=root, phase="train", gt_size=32, use_hflip=True, use_rot=True)
    opt.update(over)
    return build_dataset(opt)


def test_host_and_device_samples_of_one_seeded_index_carry_the_same_kernel(png_folder):
    from basicsr.data import degradations as G
    from basicsr.data import filter2d_host

    host, dev = _set(BLUR, png_folder, blur_kernel_size=7), _set(BLUR, png_folder, blur_kernel_size=7, blur_backend="device")
    assert type(host).__name__ == BLUR and len(host) == 3
    for index in range(3):
        _seed(40 + index)
        h = host[index]
        _seed(40 + index)
        d = dev[index]
        assert sorted(h) == ["gt", "gt_path", "lq", "lq_path"] and sorted(d) == ["blur_kernel", "gt", "gt_path", "lq_path"]
        assert torch.equal(h["gt"], d["gt"]) and tuple(d["gt"].shape) == (3, 32, 32)
        k = d["blur_kernel"]
        assert k.dtype == torch.float32 and tuple(k.shape) == (7, 7) and abs(float(k.double().sum()) - 1) < 1e-6
        assert torch.equal(h["lq"].view(torch.int32), filter2d_host(d["gt"], k).view(torch.int32))
        assert torch.equal(h["lq"].view(torch.int32), R.filter2d_f32(d["gt"][None].numpy(), k[None].numpy())[0].view(torch.int32))
        assert not torch.equal(h["lq"], h["gt"])
    # the draws after the crop and the augmentation are random_mixed_kernels' with the set's options, from the process-wide generators
    _seed(40)
    d = dev[0]
    _seed(40)
    host._gt(0)
    want = G.random_mixed_kernels(list(host.KINDS), [1 / 6] * 6, 7, [0.2, 3], [0.2, 3], [-math.pi, math.pi], [0.5, 4], [1, 2], noise_range=None)
    assert torch.equal(d["blur_kernel"], torch.from_numpy(want.astype(np.float32)))


def test_kernel_seed_repeats_and_sinc_kernels(png_folder):
    from basicsr.data import degradations as G

    val = _set(BLUR, png_folder, phase="val", blur_backend="device", kernel_seed=9, kernel_list=["aniso", "plateau_aniso"], kernel_prob=[0.7, 0.3],
               blur_sigma=[0.5, 4], betap_range=[0.8, 3])
    _seed(1)
    a = [val[i]["blur_kernel"] for i in range(3)]
    _seed(2)
    b = [val[i]["blur_kernel"] for i in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], a[1]) and tuple(a[0].shape) == (21, 21)
    want = G.random_mixed_kernels(["aniso", "plateau_aniso"], [0.7, 0.3], 21, [0.5, 4], [0.5, 4], [-math.pi, math.pi], [0.5, 4], [0.8, 3],
                                  rng=(random.Random(9 + 2), np.random.RandomState(9 + 2)))
    assert torch.equal(a[2], torch.from_numpy(want.astype(np.float32)))
    assert tuple(val[2]["gt"].shape) == (3, 64, 35)                     # other phases: the whole image
    state = random.getstate()
    val[0]
    assert random.getstate() == state                                   # a seeded set leaves the process-wide generator alone
    sinc = _set(BLUR, png_folder, phase="val", blur_backend="device", kernel_seed=3, sinc_prob=1.0, blur_kernel_size=13)
    rs = np.random.RandomState(3 + 1)
    assert rs.uniform() < 1.0
    want = G.circular_lowpass_kernel(rs.uniform(math.pi / 3, math.pi), 13)
    k = sinc[1]["blur_kernel"]
    assert torch.equal(k, torch.from_numpy(want.astype(np.float32))) and float(k.min()) < 0   # a sinc kernel has negative lobes


def test_bad_options_raise(png_folder):
    for over, text in [(dict(blur_kernel_size=20), "blur_kernel_size"), (dict(blur_kernel_size=1), "blur_kernel_size"),
                       (dict(blur_kernel_size=53), "blur_kernel_size"), (dict(blur_backend="gpu"), "blur_backend"),
                       (dict(kernel_list=["iso", "skew"]), "kernel_list"), (dict(kernel_list=["iso"], kernel_prob=[0.5, 0.5]), "kernel_prob"),
                       (dict(blur_sigma=[3, 0.2]), "blur_sigma"), (dict(betag_range=[1]), "betag_range"), (dict(sinc_prob=1.5), "sinc_prob"),
                       (dict(gt_size=10, blur_kernel_size=21), "gt_size")]:
        with pytest.raises(ValueError, match=text):
            _set(BLUR, png_folder, **over)
    small = _set(BLUR, png_folder, phase="val", center_crop=20, blur_kernel_size=41)
    with pytest.raises(ValueError, match="must exceed"):
        small[0]


# ---- mixed batches --------------------------------------------------------------------------------------------
def test_degrade_collate_with_a_blur_set(png_folder):
    from basicsr.data import DEGRADE_KINDS, degrade_collate

    assert [k for k, _ in DEGRADE_KINDS] == ["lq", "noise_sigma", "jpeg_quality", "mosaic", "inpaint_meta", "blur_kernel"]
    blur = _set(BLUR, png_folder, blur_backend="device", blur_kernel_size=7)
    noise = _set("PairedImageDenoiseDataset", png_folder, sigma_range=25, noise_backend="device")
    paired = _set("PairedImageDataset", png_folder)
    _seed(77)
    samples = [blur[0], noise[1], paired[2], blur[2], blur[1]]
    batch = degrade_collate([dict(s) for s in samples])
    assert batch["degrade_kind"].tolist() == [5, 1, 0, 5, 5] and batch["degrade_kind"].dtype == torch.int32
    assert tuple(batch["gt"].shape) == (5, 3, 32, 32) and tuple(batch["blur_kernel"].shape) == (3, 7, 7)
    for row, i in enumerate((0, 3, 4)):
        assert torch.equal(batch["blur_kernel"][row], samples[i]["blur_kernel"])
    assert tuple(batch["lq"].shape) == (1, 3, 32, 32) and tuple(batch["noise_sigma"].shape) == (1,)
    # a batch of the blur set alone is the default collate
    alone = degrade_collate([dict(samples[0]), dict(samples[3])])
    assert "degrade_kind" not in alone and tuple(alone["blur_kernel"].shape) == (2, 7, 7)
    # kernels of different sizes cannot be stacked
    other = _set(BLUR, png_folder, blur_backend="device", blur_kernel_size=9)
    with pytest.raises(ValueError, match="same blur_kernel_size"):
        degrade_collate([dict(samples[0]), dict(samples[1]), dict(other[0])])


def test_feed_data_on_a_cpu_model_raises_the_no_cpu_fallback_error(png_folder):
    """a blur batch on a model without a device reaches the op, which refuses: no fallback"""
    from basicsr.models.base_model import BaseModel
    from dcpt_amd import _lib

    m = BaseModel(dict(num_gpu=0, is_train=False))
    gt = keyed_input("blurcpu.feed", (2, 3, 16, 16))
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        m._lq_on_device({"gt": gt, "blur_kernel": torch.full((2, 3, 3), 1 / 9)})
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        m._lq_on_device({"gt": gt, "degrade_kind": torch.tensor([5, 5], dtype=torch.int32), "blur_kernel": torch.full((2, 3, 3), 1 / 9)})
    with pytest.raises(ValueError, match="0..5"):
        m._lq_on_device({"gt": gt, "degrade_kind": torch.tensor([0, 6], dtype=torch.int32), "lq": gt})
