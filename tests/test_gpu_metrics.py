"""GPU: the device-side validation metrics (dcpt_amd/csrc/metrics.hip through DF.image_metric_sums, basicsr.metrics.calculate_psnr_device /
calculate_ssim_device / MetricSums, and ``val.device_metrics`` of SRModel.nondist_validation) against the yardstick they mirror: the host
functions ``calculate_psnr`` / ``calculate_ssim`` fed the same fp32 arrays, and for PSNR the reference's own values in
tests/golden/metrics.npz.

Tolerances (derived, not tuned):
* PSNR, quantised RGB / gray path: ``==``.  The squared error is an exact integer on both sides (int64 on the device) and both sides
  finish it with the same numpy expression.
* PSNR, luma / image_range = 1 paths: 1e-6 dB.  An fp64 sum in another order moves it by ~1e-14 relative; a one-ulp flip of one luma
  value's fp32 rounding would move it by ~1e-8 dB.
* PSNR against the golden: 1e-9, the bound the host function meets.
* SSIM: 1e-10 absolute.  Windowed moments of values up to 255^2 carry ~1e-11 of absolute fp64 error after the E[x^2] - mu^2 cancellation
  and are divided by a denominator >= C2 = 58.5; only the summation order differs between the two sides.

Worst measured difference: see ``test_grid_matches_host``."""
import os

import numpy as np
import pytest
import torch

from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSNR_TOL, SSIM_TOL = 1e-6, 1e-10
TH, TW = 16, 32   # DF.METRIC_TILE (asserted below: the shapes here are aimed at these edges)
# cropped sizes: one map position; one row; a ragged small one; the plumbing test's 40 x 37; one short of / one past a tile edge in each
# direction; two tile rows exactly
SHAPES = [(11, 11), (11, 50), (12, 37), (40, 37), (TH + 9, TW + 11), (TH + 11, TW + 9), (2 * TH + 10, TW + 10)]


def _cases():
    """a thinned product: every shape with all four (test_y_channel, image_range) pairs, B / C / crop_border rotating so that every value of
    every axis meets every shape's neighbours -- including luma on C = 3 and the luma flag on C = 1 (where it does nothing)"""
    out = []
    for i, (hc, wc) in enumerate(SHAPES):
        for y in (False, True):
            for rng in (255, 1):
                r = int(rng == 1)
                out.append(dict(hc=hc, wc=wc, B=(1, 3)[(i + y) % 2], C=(3, 1)[(i + r + (i // 2) * y) % 2], crop=(0, 3)[(i + y + r) % 2], y=y, rng=rng))
    return out


CASES = _cases()
_id = lambda c: f"{c['hc']}x{c['wc']}-B{c['B']}C{c['C']}-cb{c['crop']}-y{int(c['y'])}-r{c['rng']}"  # noqa: E731


def test_case_grid_covers_every_axis():
    from dcpt_amd import functional as DF

    assert DF.METRIC_TILE == (TH, TW)
    for k, vals in dict(B=(1, 3), C=(1, 3), crop=(0, 3), y=(False, True), rng=(255, 1)).items():
        assert {c[k] for c in CASES} == set(vals), k
    assert {(c["hc"], c["wc"]) for c in CASES} == set(SHAPES)
    for rng in (255, 1):
        assert any(c["y"] and c["C"] == 3 and c["rng"] == rng for c in CASES) and any(c["y"] and c["C"] == 1 and c["rng"] == rng for c in CASES)
        assert any(not c["y"] and c["C"] == 3 and c["rng"] == rng for c in CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _pair(tag, shape):
    """keyed uniform image + bounded noise clipped to [0, 1], as the golden's inputs"""
    a = keyed_input(f"{tag}.a", shape).numpy()
    b = np.clip(a + keyed_input(f"{tag}.n", shape, lo=-0.08, hi=0.08).numpy(), 0, 1).astype(np.float32)
    return a, b


def _tie_pair(shape):
    """every value is (j + 0.5) / 255: where x * 255 lands on j + 0.5 in fp32 the rounding mode (half to even) decides the uint8 value"""
    n = int(np.prod(shape))
    j = (np.arange(n, dtype=np.int64) * 7) % 256
    a = ((j + 0.5) / 255.0).astype(np.float32).reshape(shape)
    b = ((((j * 3 + 1) % 256) + 0.5) / 255.0).astype(np.float32).reshape(shape)
    return np.minimum(a, 1.0), np.minimum(b, 1.0)


def _host(a, b, crop, y, rng, ssim=True):
    from basicsr.metrics import calculate_psnr, calculate_ssim

    return (calculate_psnr(a, b, crop, test_y_channel=y, image_range=rng),
            calculate_ssim(a, b, crop, test_y_channel=y, image_range=rng) if ssim else None)


def _device(a, b, crop, y, rng, dev):
    from basicsr.metrics import calculate_psnr_device, calculate_ssim_device

    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    return (calculate_psnr_device(ta, tb, crop, test_y_channel=y, image_range=rng),
            calculate_ssim_device(ta, tb, crop, test_y_channel=y, image_range=rng))


def _compare(case, a, b, dev):
    crop, y, rng = case["crop"], case["y"], case["rng"]
    hp, hs = _host(a, b, crop, y, rng)
    dp, ds = _device(a, b, crop, y, rng, dev)
    exact = rng == 255 and not (y and a.shape[1] == 3)
    dpsnr = 0.0 if hp == dp else abs(hp - dp)
    print(f"metrics {_id(case)}: psnr host {hp!r} device {dp!r} |d| {dpsnr:.3e} ({'==' if exact else '1e-6'});  "
          f"ssim host {hs!r} device {ds!r} |d| {abs(hs - ds):.3e}")
    if exact:
        assert dp == hp, (case, hp, dp)
    else:
        assert dpsnr <= PSNR_TOL, (case, hp, dp)
    assert abs(hs - ds) <= SSIM_TOL, (case, hs, ds)
    return dpsnr, abs(hs - ds)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_grid_matches_host(case, dev):
    """device PSNR / SSIM against the host functions on the same fp32 arrays.  Worst difference: NOT YET MEASURED on the MI355X (no
    device was available when this was written; each case prints its figures before it asserts).  A numpy restatement of the kernel's
    tiling, ownership rule and operation order, run on the host over five of these shapes, differed from the host functions by at most
    4.6e-14 dB (PSNR, luma / image_range = 1 paths; 0 on the exact path) and 4.4e-16 (SSIM)."""
    H, W = case["hc"] + 2 * case["crop"], case["wc"] + 2 * case["crop"]
    a, b = _pair(f"gpumetrics.{case['hc']}x{case['wc']}", (case["B"], case["C"], H, W))
    _compare(case, a, b, dev)


@pytest.mark.parametrize("y", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_tie_image_rounds_half_to_even(C, y, dev):
    a, b = _tie_pair((1, C, 40, 37))
    q = a.astype(np.float32) * np.float32(255.0)
    assert int((q == np.floor(q) + 0.5).sum()) > 100, "the tie image has no ties in fp32: the rounding mode would not matter"
    _compare(dict(hc=40, wc=37, B=1, C=C, crop=0, y=y, rng=255), a, b, dev)


def test_psnr_matches_reference_fixture(dev):
    """the reference's own ``calculate_psnr`` (tests/golden/metrics.npz), inputs rebuilt as tests/test_plumbing_cpu.py does"""
    from basicsr.metrics import calculate_psnr, calculate_psnr_device

    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))
    a = keyed_input("metrics.a", (2, 3, 24, 20)).numpy()
    b = np.clip(a + keyed_input("metrics.n", (2, 3, 24, 20), lo=-0.08, hi=0.08).numpy(), 0, 1).astype(np.float32)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for cb in (0, 3):
        for ych in (False, True):
            mine = calculate_psnr_device(ta, tb, cb, test_y_channel=ych, image_range=255.0)
            print(f"golden psnr_cb{cb}_y{int(ych)}: device {mine!r} golden {float(g[f'psnr_cb{cb}_y{int(ych)}'])!r}")
            assert abs(mine - float(g[f"psnr_cb{cb}_y{int(ych)}"])) < 1e-9, (cb, ych, mine)
            if not ych:
                assert mine == calculate_psnr(a, b, cb, test_y_channel=ych, image_range=255.0)
    assert abs(calculate_psnr_device(ta, tb, 0, image_range=1) - float(g["psnr_range1"])) < 1e-9
    single = calculate_psnr_device(ta[:1], tb[:1], 2, image_range=255.0)
    assert abs(single - float(g["psnr_single_chw"])) < 1e-9 and single == calculate_psnr(a[0], b[0], 2, image_range=255.0)
    assert calculate_psnr_device(ta, ta.clone(), 0) == float("inf") and np.isinf(g["psnr_equal"])


@pytest.mark.parametrize("y, rng", [(False, 255), (True, 255), (False, 1)])
def test_identical_images(y, rng, dev):
    from basicsr.metrics import calculate_psnr_device, calculate_ssim_device

    a = torch.from_numpy(_pair("gpumetrics.same", (3, 3, TH + 11, TW + 11))[0]).to(dev)
    assert calculate_psnr_device(a, a.clone(), 0, test_y_channel=y, image_range=rng) == float("inf")
    assert abs(calculate_ssim_device(a, a.clone(), 0, test_y_channel=y, image_range=rng) - 1.0) <= 1e-12


def test_two_calls_give_identical_bits_and_noncontiguous_inputs_are_taken(dev):
    from dcpt_amd import functional as DF

    a, b = (torch.from_numpy(t).to(dev) for t in _pair("gpumetrics.bits", (3, 3, 2 * TH + 13, 2 * TW + 13)))
    for y, rng in ((False, 255), (True, 255), (False, 1)):
        r1 = DF.image_metric_sums(a, b, 1, y, rng)
        r2 = DF.image_metric_sums(a, b, 1, y, rng)
        assert r1[0].dtype == (torch.int64 if (rng == 255 and not y) else torch.float64) and r1[1].dtype == torch.float64
        assert tuple(r1[0].shape) == (3,) and tuple(r1[1].shape) == (3, 1 if y else 3)
        assert torch.equal(r1[0].view(torch.int64), r2[0].view(torch.int64)) and torch.equal(r1[1].view(torch.int64), r2[1].view(torch.int64))
        # a channels_last view / a sliced view of a larger tensor: .contiguous() inside, the same bits out
        r3 = DF.image_metric_sums(a.contiguous(memory_format=torch.channels_last), torch.cat([b, b], 3)[..., : b.shape[3]], 1, y, rng)
        assert torch.equal(r1[0].view(torch.int64), r3[0].view(torch.int64)) and torch.equal(r1[1].view(torch.int64), r3[1].view(torch.int64))
    sse, none = DF.image_metric_sums(a, b, 1, ssim=False)
    assert none is None and torch.equal(sse, DF.image_metric_sums(a, b, 1)[0])
    small = DF.image_metric_sums(a[..., :8, :9], b[..., :8, :9], 0, ssim=False)[0]   # PSNR alone has no 11-pixel minimum
    qa, qb = (a[..., :8, :9] * 255.0).round().long(), (b[..., :8, :9] * 255.0).round().long()
    assert torch.equal(small, ((qa - qb) ** 2).sum(dim=(1, 2, 3)))


def test_accumulator_matches_single_calls(dev):
    """MetricSums over three batches of different shapes: one transfer at the end, the per-batch values of the single-call functions"""
    from basicsr.metrics import MetricSums, calculate_psnr_device, calculate_ssim_device

    acc = MetricSums(crop_border=3, test_y_channel=True)
    pairs = []
    for k, shape in enumerate([(1, 3, 30, 41), (2, 3, 17, 64), (1, 1, 48, 48)]):
        pairs.append(tuple(torch.from_numpy(t).to(dev) for t in _pair(f"gpumetrics.acc{k}", shape)))
        acc.add(*pairs[-1])
    res = acc.result()
    assert res["psnr"] == [calculate_psnr_device(a, b, 3, test_y_channel=True) for a, b in pairs]
    assert res["ssim"] == [calculate_ssim_device(a, b, 3, test_y_channel=True) for a, b in pairs]


def test_stays_inside_its_buffers(dev):
    from redzone import redzone

    from dcpt_amd import functional as DF

    a, b = (torch.from_numpy(t).to(dev) for t in _pair("gpumetrics.rz", (3, 3, TH + 11 + 6, TW + 9 + 6)))
    ref = [DF.image_metric_sums(a, b, 3, y, rng) for y, rng in ((False, 255), (True, 1))]
    with redzone() as rz:
        got = [DF.image_metric_sums(a, b, 3, y, rng) for y, rng in ((False, 255), (True, 1))]
    assert rz.count > 0
    for (s0, m0), (s1, m1) in zip(ref, got):   # (a workspace that starts as NaNs: nothing unwritten is read)
        assert torch.equal(s0.view(torch.int64), s1.view(torch.int64)) and torch.equal(m0.view(torch.int64), m1.view(torch.int64))


def test_launch_trace_names_the_metric_kernels(dev):
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    a, b = (torch.from_numpy(t).to(dev) for t in _pair("gpumetrics.trace", (1, 3, 24, 24)))
    with kernel_trace() as t:
        DF.image_metric_sums(a, b)
        DF.image_metric_sums(a, b, ssim=False)
    t.assert_ran("metric.tile_ssim", "metric.tile_psnr", "metric.reduce")
    assert t["metric.reduce"] == 2 and set(t.families()) == set(t.families("metric."))


def test_bad_arguments_raise(dev):
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    a = torch.rand(1, 3, 16, 16, device=dev)
    with pytest.raises(_lib.DcptHipError, match="at least 11 x 11"):
        DF.image_metric_sums(a, a, 3)
    with pytest.raises(_lib.DcptHipError, match="C must be 1 or 3"):
        DF.image_metric_sums(a[:, :2], a[:, :2])
    with pytest.raises(ValueError):
        DF.image_metric_sums(a, a, image_range=65535)


# ---- SRModel.nondist_validation -------------------------------------------------------------------------------------------------------
TINY = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1])


def _validate(device_metrics, clamp=True, save_img=False, tmp_path=None, metrics=None):
    from basicsr.data import build_dataloader, build_dataset
    from basicsr.models import build_model
    from dcpt_amd.keyed_init import fill_module_

    val = dict(save_img=save_img, metrics=metrics or dict(psnr=dict(type="calculate_psnr", crop_border=0, test_y_channel=False),
                                                          ssim=dict(type="calculate_ssim", crop_border=0, test_y_channel=False)))
    if device_metrics is not None:
        val["device_metrics"] = device_metrics
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="NAFNetBaseline", window_size=16, **TINY), path=dict(pretrain_network_g=None, visualization=str(tmp_path)),
               val=val)
    m = build_model(opt)
    fill_module_(m.net_g)
    dopt = dict(name="syn", type="SyntheticPairedDataset", phase="val", num=2, size=(40, 37), seed=3)
    loader = build_dataloader(build_dataset(dopt), dopt)
    return m, loader


def test_validation_device_route_matches_host_route(dev, monkeypatch, tmp_path):
    from basicsr.models.sr_model import SRModel

    m0, loader = _validate(None)
    host = dict(m0.nondist_validation(loader, 1, None, False))
    assert np.isfinite(host["psnr"]) and np.isfinite(host["ssim"]) and host["ssim"] < 1

    m1, loader = _validate(True)
    calls = []
    monkeypatch.setattr(SRModel, "get_current_visuals", lambda self: calls.append(1) or (_ for _ in ()).throw(AssertionError("get_current_visuals called")))
    got = dict(m1.nondist_validation(loader, 1, None, False))
    print(f"validation: host {host} device {got}")
    assert not calls
    assert got["psnr"] == host["psnr"] and abs(got["ssim"] - host["ssim"]) <= SSIM_TOL
    assert list(got) == list(host) and m1.metric_results == got
    monkeypatch.undo()

    # save_img: only the result travels to the host, and the same picture is written
    from PIL import Image

    (tmp_path / "h").mkdir()
    (tmp_path / "d").mkdir()
    mh, loader = _validate(None, save_img=True, tmp_path=tmp_path / "h")
    mh.nondist_validation(loader, 1, None, True)
    md, loader = _validate(True, save_img=True, tmp_path=tmp_path / "d")
    monkeypatch.setattr(SRModel, "get_current_visuals", lambda self: (_ for _ in ()).throw(AssertionError("get_current_visuals called")))
    assert dict(md.nondist_validation(loader, 1, None, True)) == got
    files = sorted(p.name for p in (tmp_path / "h" / "syn").iterdir())
    assert len(files) == 2 and files == sorted(p.name for p in (tmp_path / "d" / "syn").iterdir())
    for f in files:
        assert np.array_equal(np.asarray(Image.open(tmp_path / "h" / "syn" / f)), np.asarray(Image.open(tmp_path / "d" / "syn" / f)))


def test_validation_without_clamp_or_with_other_metrics_stays_on_the_host(dev, monkeypatch):
    from dcpt_amd import functional as DF

    m0, loader = _validate(None)
    host = dict(m0.nondist_validation(loader, 1, None, False, clamp=False))
    m1, loader = _validate(True)
    real = DF.image_metric_sums
    monkeypatch.setattr(DF, "image_metric_sums", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device metrics without clamp")))
    seen = []
    visuals = type(m1).get_current_visuals
    monkeypatch.setattr(type(m1), "get_current_visuals", lambda self: seen.append(1) or visuals(self))
    assert dict(m1.nondist_validation(loader, 1, None, False, clamp=False)) == host and len(seen) == 2
    # a metric the kernel does not mirror (BHWC order is refused by the device functions; image_range 65535 is not 255 / 1) keeps the host
    # function while its neighbour goes to the device
    monkeypatch.setattr(DF, "image_metric_sums", real)
    mixed = dict(psnr=dict(type="calculate_psnr", crop_border=2, test_y_channel=True),
                 psnr16=dict(type="calculate_psnr", crop_border=2, image_range=65535))
    mh, loader = _validate(None, metrics=mixed)
    want = dict(mh.nondist_validation(loader, 1, None, False))
    md, loader = _validate(True, metrics=mixed)
    assert md._device_metric_plan(mixed, True) == {"psnr": ((2, True, 255), "psnr")} and md._device_metric_plan(mixed, False) == {}
    got = dict(md.nondist_validation(loader, 1, None, False))
    assert got["psnr16"] == want["psnr16"] and abs(got["psnr"] - want["psnr"]) <= PSNR_TOL
