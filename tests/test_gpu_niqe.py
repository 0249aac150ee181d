"""GPU: the NIQE kernels and the MATLAB-bicubic resize of dcpt_amd/csrc/niqe.hip (dcpt_imresize_fwd, dcpt_niqe_mscn_fwd,
dcpt_niqe_block_stats_fwd) behind dcpt_amd.functional and basicsr.metrics.calculate_niqe_device / NiqeSums.

Yardstick.  The truth T is the kernel-blind restatement (tests/niqe_restatement.py) in ``np.longdouble``.  The kernels are fp64 arithmetic
in another summation order, so they are held to a small multiple of what fp64 itself loses, measured on the same input:

    max|kernel - T|  <=  4 * max|float64 restatement - T|  +  1e-13 * max|T|

for the MSCN planes, the resize output and the sums of the stats tensor.  The counts are compared exactly, except that an element with
0 < |T| < 1e-9 may take either sign: per block and map the counts may differ by at most the number of such elements, which the fixture
images keep under 0.1 % of a block (they hold none; the exact zeros of case (c)'s constant corner are exact zeros on both sides).  Scores against the
reference's own (tests/golden/niqe.npz) use the CPU test's bound.

Measured on one MI355X (kernel / float64 restatement / bound): MSCN scale 1 3.6e-15 / 1.3e-14 / 2.2e-13, the x0.5 image 3.0e-16 / 3.3e-16 /
6.7e-14, MSCN scale 2 1.9e-14 / 2.5e-14 / 2.5e-13, the sums 9.1e-13 / 5.8e-13 / 3.1e-10 at max|T| 3.1e3; imresize 0 on the dyadic scales
(every weight and product is exact) and 3.5e-16 / 3.5e-16 / 7.8e-14 at 1/3; no count differs."""
import os

import numpy as np
import pytest
import torch

import niqe_restatement as R
from test_niqe_cpu import GOLDEN, PRIS, RESIZE_CASES, RESIZE_TOL, SCORE_RTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "niqe.npz")) as f:
        d = {k: f[k] for k in f.files}
    for tag in "abc":
        d[f"{tag}.img"] = R.decode_planes(d[f"{tag}.planes_dx"]).astype(np.float32) / np.float32(255.0)
    return d


@pytest.fixture(scope="module")
def resize_gold():
    with np.load(os.path.join(GOLDEN, "imresize.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def truth(gold):
    """per case: (T, the float64 restatement), computed once and shared"""
    return {tag: (R.pipeline(gold[f"{tag}.img"], 0, np.longdouble), R.pipeline(gold[f"{tag}.img"], 0, np.float64)) for tag in "abc"}


def _held(name, k, T, r64):
    """the yardstick; prints the three numbers"""
    T = np.asarray(T)
    ek = float(np.abs(np.asarray(k, dtype=np.longdouble) - T).max())
    er = float(np.abs(np.asarray(r64, dtype=np.longdouble) - T).max())
    mt = float(np.abs(T).max())
    bound = 4 * er + 1e-13 * mt
    print(f"{name}: kernel {ek:.3e}, float64 restatement {er:.3e}, max|T| {mt:.3e} (bound {bound:.3e})")
    assert ek <= bound, f"{name}: {ek:.3e} above {bound:.3e}"


# ---- the pipeline against the longdouble truth ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_planes_and_sums_against_longdouble(dev, gold, truth, tag):
    from dcpt_amd import functional as DF

    T, r64 = truth[tag]
    stats, parts = DF.niqe_stats(torch.from_numpy(gold[f"{tag}.img"]).to(dev), 0, parts=True)
    stats = stats.cpu().numpy()
    assert stats.shape == T["stats"].shape and stats.dtype == np.float64
    for key in ("mscn1", "img2", "mscn2"):
        _held(f"{tag} {key}", parts[key].cpu().numpy(), T[key], r64[key])
    sums = [1, 3, 4, 5]
    _held(f"{tag} sums", stats[..., sums], T["stats"][..., sums], r64["stats"][..., sums])
    # counts: exact, up to the elements whose sign is undecided
    for s, (key, bs) in enumerate((("mscn1", 96), ("mscn2", 48))):
        for p, plane in enumerate(T[key]):
            for k, maps in R.block_maps(plane, bs):
                for m, v in enumerate(maps):
                    tiny = int(((np.abs(v) < 1e-9) & (v != 0)).sum())   # (an exact 0 of T -- a constant window -- is one of the kernel too)
                    assert tiny <= 0.001 * bs * bs, f"the fixture image holds {tiny} undecided elements in one block"
                    for c in (0, 2):
                        diff = abs(stats[p, k, s, m, c] - float(T["stats"][p, k, s, m, c]))
                        assert diff <= tiny, f"{tag} plane {p} block {k} scale {s + 1} map {m}: count off by {diff}"


def test_flat_block_is_bitwise_zero(dev, gold, truth):
    """case (c): the first block is constant.  The kernel's MSCN is bitwise +-0 there at both scales, its resize bitwise constant, the
    counts and sums exactly zero on both sides"""
    from dcpt_amd import functional as DF

    T, _ = truth["c"]
    stats, parts = DF.niqe_stats(torch.from_numpy(gold["c.img"]).to(dev), 0, parts=True)
    assert not bool(parts["mscn1"][0, :96, :96].any()) and not bool(parts["mscn2"][0, :48, :48].any())
    assert len(torch.unique(parts["img2"][0, :51, :51])) == 1     # (the 48 x 48 block and the 3-wide reach of its windows)
    assert not bool(stats[0, 0].any()) and not np.any(T["stats"][0, 0])
    assert bool(stats[0, 1:].any())


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_scores_match_the_reference(dev, gold, tag):
    from basicsr.metrics import calculate_niqe, calculate_niqe_device

    img, ref = gold[f"{tag}.img"], float(gold[f"{tag}.score"])
    got = calculate_niqe_device(torch.from_numpy(img).to(dev), 0, pris_params=PRIS)
    host = calculate_niqe(img, 0, pris_params=PRIS)
    print(f"niqe {tag}: device {got:.9f}, host {host:.9f}, reference {ref:.9f}: relative {abs(got - ref) / ref:.3e} (bound {SCORE_RTOL:.3e})")
    assert abs(got - ref) <= SCORE_RTOL * abs(ref)


def test_crop_border_on_the_device(dev, gold):
    """case (d): the spatial crop is addressing; the score is the restatement's on the cropped planes (1e-8: see tests/test_niqe_cpu.py)"""
    from basicsr.metrics import calculate_niqe_device

    with np.load(PRIS) as f:
        mu, cov = f["mu_pris_param"].astype(np.float64), f["cov_pris_param"].astype(np.float64)
    got = calculate_niqe_device(torch.from_numpy(gold["b.img"]).to(dev), 4, pris_params=PRIS)
    want = R.niqe(gold["b.img"], 4, mu, cov)
    print(f"niqe d: device {got:.12f}, restatement {want:.12f}")
    assert abs(got - want) <= 1e-8 * abs(want)


# ---- imresize --------------------------------------------------------------------------------------------------------------------------
def _resize_case(dev, x_chw, scale, aa, name, ref=None):
    from dcpt_amd import functional as DF

    T = R.imresize_planes(x_chw, scale, aa, np.longdouble)
    r64 = R.imresize_planes(x_chw, scale, aa, np.float64)
    xd = torch.from_numpy(np.ascontiguousarray(x_chw)).to(dev)[None]
    y64 = DF.imresize(xd, scale, aa, out_dtype=torch.float64)[0].cpu().numpy()
    y64_from64 = DF.imresize(xd.double(), scale, aa)[0].cpu().numpy()
    y32 = DF.imresize(xd, scale, aa)[0].cpu().numpy()
    assert y64.shape == T.shape and y32.dtype == np.float32 and y64_from64.dtype == np.float64
    _held(f"imresize {name}", y64, T, r64)
    assert np.array_equal(y64, y64_from64)       # (an fp32 value is the same number as fp64 input)
    t32 = T.astype(np.float32)
    ulp = np.spacing(np.abs(t32))
    assert np.all(np.abs(y32.astype(np.float64) - t32.astype(np.float64)) <= ulp), f"imresize {name}: fp32 output off by more than one ulp"
    if ref is not None:
        assert np.abs(y32.astype(np.float64) - ref).max() <= RESIZE_TOL
    return y32


@pytest.mark.parametrize("tag", RESIZE_CASES)
def test_imresize_against_longdouble_and_the_reference(dev, resize_gold, tag):
    from basicsr.utils import imresize

    g = resize_gold
    h, w = (int(v) for v in g[f"{tag}.size"])
    x = g[f"x.{h}x{w}"].transpose(2, 0, 1)
    scale, aa = float(g[f"{tag}.scale"]), bool(g[f"{tag}.antialiasing"])
    y32 = _resize_case(dev, x, scale, aa, tag, g[f"{tag}.y_chw"])
    # the reference's interface on a device tensor: (c, h, w) and (h, w), float32
    y = imresize(torch.from_numpy(np.ascontiguousarray(x)).to(dev), scale, antialiasing=aa)
    assert y.is_cuda and y.dtype == torch.float32 and np.array_equal(y.cpu().numpy(), y32)
    assert np.array_equal(imresize(torch.from_numpy(np.ascontiguousarray(x[0])).to(dev), scale, antialiasing=aa).cpu().numpy(), y32[0])


def test_imresize_where_every_tap_reflects(dev, resize_gold):
    """1 x 1 x 8 x 8 at 0.5: the 10 taps of every output sample reach outside an 8-pixel axis on one side or both"""
    _resize_case(dev, resize_gold["x.8x8"].transpose(2, 0, 1)[:1], 0.5, True, "1x1x8x8")
    from dcpt_amd import functional as DF

    with pytest.raises(ValueError, match="shorter than the kernel reaches"):
        DF.imresize(torch.zeros(1, 1, 2, 16, device=dev), 0.5)


# ---- consistency -------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_single_planes_and_runs_repeat(dev, gold):
    from dcpt_amd import functional as DF

    img = torch.from_numpy(gold["a.img"]).to(dev)        # 2 x 1 x 192 x 96
    both = DF.niqe_stats(img, 0)
    for b in range(2):
        assert torch.equal(DF.niqe_stats(img[b:b + 1], 0).view(torch.int64), both[b:b + 1].view(torch.int64))
    assert torch.equal(DF.niqe_stats(img, 0).view(torch.int64), both.view(torch.int64))
    x = torch.from_numpy(gold["b.img"]).to(dev)
    y1, y2 = DF.imresize(x, 1 / 3), DF.imresize(x, 1 / 3)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
    s1, p1 = DF.niqe_stats(x, 4, parts=True)
    s2, p2 = DF.niqe_stats(x, 4, parts=True)
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64)) and all(torch.equal(p1[k].view(torch.int64), p2[k].view(torch.int64)) for k in p1)
    assert torch.equal(DF.niqe_stats(x, 4).view(torch.int64), s1.view(torch.int64))   # (without parts the MSCN buffer is reused: same bits)


def _resize_args(dev, P, H, W, scale):
    from dcpt_amd import functional as DF

    (fh, wh), (fw, ww) = DF._resize_tables(H, scale, True, dev), DF._resize_tables(W, scale, True, dev)
    return (fh, wh, fw, ww), (P, H, W, fh.numel(), fw.numel(), wh.shape[1], ww.shape[1])


def test_exact_workspace_is_accepted_and_a_short_one_refused(dev, gold):
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    x = torch.from_numpy(gold["a.img"]).to(dev).view(2, 192, 96)
    tabs, geo = _resize_args(dev, 2, 192, 96, 0.5)
    need = lib.dcpt_imresize_ws_bytes(*geo)
    assert need == 2 * 96 * 96 * 8
    y = torch.empty(2, 96, 48, dtype=torch.float64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = DF._stream(dev)
    args = lambda n: (x.data_ptr(), y.data_ptr(), *(t.data_ptr() for t in tabs), ws.data_ptr(), n, *geo, 192 * 96, 96, DF.IMRESIZE_Y_F64, st)
    assert lib.dcpt_imresize_fwd(*args(need)) == 0
    assert lib.dcpt_imresize_fwd(*args(need - 1)) != 0 and "workspace too small" in lib.dcpt_last_error().decode()
    assert torch.equal(y, DF.imresize(x[None], 0.5, out_dtype=torch.float64)[0])


def test_stays_inside_its_buffers(dev, gold):
    """every entry point on buffers of exactly the size it asks for, with guards behind the outputs and the workspace (all start as NaN
    patterns: nothing unwritten is read); ragged crop (case (b) with crop_border 4), the bits of the ordinary route"""
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    img = torch.from_numpy(gold["b.img"]).to(dev)
    want, parts = DF.niqe_stats(img, 4, parts=True)
    planes = img.view(3, 200, 300)
    f64 = lambda buf, *shape: buf.view(torch.float64).view(*shape)
    with redzone() as rz:
        n1 = DF.niqe_mscn(planes, 4, 1, out=f64(DF._workspace(dev, 3 * 192 * 288 * 8), 3, 192, 288))
        s1 = DF.niqe_block_stats(n1, 96, out=f64(DF._workspace(dev, 3 * 6 * 30 * 8), 3, 6, 5, 6))
        x2 = f64(DF._workspace(dev, 3 * 96 * 144 * 8), 3, 96, 144)
        DF._imresize_planes(planes[:, 4:, 4:], 3, 192, 288, 200 * 300, 300, 0.5, True, x2, DF.IMRESIZE_Y_F64 | DF.IMRESIZE_QUANT8)
        n2 = DF.niqe_mscn(x2, 0, 2, out=f64(DF._workspace(dev, 3 * 96 * 144 * 8), 3, 96, 144))
        s2 = DF.niqe_block_stats(n2, 48, out=f64(DF._workspace(dev, 3 * 6 * 30 * 8), 3, 6, 5, 6))
        y32 = DF._workspace(dev, 3 * 67 * 100 * 4).view(torch.float32).view(3, 67, 100)   # the fp32 store: 200 x 300 at 1/3
        DF._imresize_planes(planes, 3, 200, 300, 200 * 300, 300, 1 / 3, True, y32, 0)
    assert rz.count == 8   # six outputs and the two resize workspaces
    bits = lambda t: t.contiguous().view(torch.int64)
    assert torch.equal(bits(n1), bits(parts["mscn1"])) and torch.equal(bits(x2), bits(parts["img2"])) and torch.equal(bits(n2), bits(parts["mscn2"]))
    assert torch.equal(bits(torch.stack((s1, s2), dim=2)), bits(want))
    assert torch.equal(y32, DF.imresize(img, 1 / 3)[0])


def test_launch_count(dev, gold):
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    img = torch.from_numpy(gold["a.img"]).to(dev)
    DF.niqe_stats(img, 0)
    with kernel_trace() as t:
        DF.niqe_stats(img, 0)
    assert t.counts == {"niqe.mscn1": 1, "niqe.stats96": 1, "imresize.h": 1, "imresize.w": 1, "niqe.mscn2": 1, "niqe.stats48": 1}, t.counts


def test_accumulator_and_refusals(dev, gold):
    from basicsr.metrics import NiqeSums, calculate_niqe_device
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    a, b = torch.from_numpy(gold["a.img"]).to(dev), torch.from_numpy(gold["b.img"]).to(dev)
    acc = NiqeSums(crop_border=0, pris_params=PRIS)
    acc.add(a)
    acc.add(b)
    acc.add(a[:1])
    assert acc.result()["niqe"] == [calculate_niqe_device(t, 0, pris_params=PRIS) for t in (a, b, a[:1])]
    with pytest.raises(ValueError, match="at least two whole"):
        calculate_niqe_device(a[:, :, :191], 0, pris_params=PRIS)
    with pytest.raises(ValueError, match="BCHW"):
        calculate_niqe_device(a, 0, input_order="BHWC", pris_params=PRIS)
    with pytest.raises(_lib.DcptHipError):
        DF.niqe_stats(a.cpu(), 0)
    with pytest.raises(_lib.DcptHipError, match="whole blocks"):
        DF.niqe_block_stats(torch.zeros(1, 100, 96, dtype=torch.float64, device=dev), 96)
    with pytest.raises(_lib.DcptHipError, match="scale 2 takes whole 48 x 48 blocks"):
        DF.niqe_mscn(torch.zeros(1, 50, 96, dtype=torch.float64, device=dev), 0, 2)


# ---- SRModel.nondist_validation ------------------------------------------------------------------------------------------------------
def test_validation_scores_niqe_on_the_device(dev, monkeypatch):
    """a tiny network over two 1 x 3 x 200 x 300 images with ``val.device_metrics: true``: the logged NIQE is the mean of
    calculate_niqe_device over the images the accumulator saw, nothing travels to the host per image (``get_current_visuals`` is never
    called, as tests/test_gpu_metrics.py asserts for PSNR / SSIM) and the two accumulators' sums make one transfer after the last image"""
    from basicsr.data import build_dataloader, build_dataset
    from basicsr.metrics import NiqeSums, calculate_niqe_device
    from basicsr.models import build_model
    from basicsr.models.sr_model import SRModel
    from dcpt_amd.keyed_init import fill_module_

    tiny = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1])
    metrics = dict(niqe=dict(type="calculate_niqe", crop_border=4, pris_params=PRIS), psnr=dict(type="calculate_psnr", crop_border=0))
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="NAFNetBaseline", window_size=16, **tiny), path=dict(pretrain_network_g=None, visualization=None),
               val=dict(save_img=False, device_metrics=True, metrics=metrics))
    m = build_model(opt)
    fill_module_(m.net_g)
    dopt = dict(name="syn", type="SyntheticPairedDataset", phase="val", num=2, size=(200, 300), seed=5)
    loader = build_dataloader(build_dataset(dopt), dopt)

    seen, events = [], []
    add, cpu = NiqeSums.add, torch.Tensor.cpu
    monkeypatch.setattr(NiqeSums, "add", lambda self, img, img2=None: (seen.append(img.clone()), events.append("add"), add(self, img, img2))[-1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (events.append("cpu"), cpu(self, *a, **k))[-1])
    monkeypatch.setattr(SRModel, "get_current_visuals", lambda self: (_ for _ in ()).throw(AssertionError("get_current_visuals called")))
    got = dict(m.nondist_validation(loader, 1, None, False))
    monkeypatch.undo()
    assert events == ["add", "add", "cpu"], events      # (one transfer for both accumulators -- NIQE, PSNR -- after the last image)
    assert len(seen) == 2 and tuple(seen[0].shape) == (1, 3, 200, 300)
    want = float(np.mean([calculate_niqe_device(t, 4, pris_params=PRIS) for t in seen]))
    print(f"validation: niqe {got['niqe']:.9f} (per image, averaged: {want:.9f}), psnr {got['psnr']:.4f}")
    assert got["niqe"] == want and np.isfinite(got["psnr"]) and list(got) == ["niqe", "psnr"]
