"""GPU: MS-SSIM, MATLAB SSIM and NRMSE on the device (dcpt_amd/csrc/metrics_ms.hip through DF.msssim_sums / ssim_matlab_sums /
image_range_minmax, basicsr.metrics.calculate_msssim_device / calculate_ssim_matlab_device / calculate_nrmse_device / MetricSums, and
``val.device_metrics`` of SRModel.nondist_validation) against the host functions ``calculate_msssim`` / ``calculate_ssim_matlab`` /
``calculate_nrmse`` fed the same fp32 arrays.

Tolerances (derived, not tuned; the per-map figure is tests/test_gpu_metrics.py's):
* per-level SSIM / CS sums divided by their counts, and MATLAB SSIM: 1e-10 absolute.  Windowed moments of values up to 255^2 carry ~1e-11
  of absolute fp64 error after the E[x^2] - mu^2 cancellation and are divided by a denominator >= C2; only the summation order differs
  between the two sides (the box blur is the same expression in the same order, exact on the quantised path).
* MS-SSIM: 1e-9.  Every case asserts on the host side that every mean entering the product is >= 0.5; the relative error of
  prod x_k^w_k is sum_k w_k 1e-10 / x_k <= 2e-10 sum_k w_k, and the value is <= 1.
* NRMSE: ``==`` on the quantised RGB / gray path (the squared error is an exact integer, minimum and maximum are exact, both sides finish
  with the same numpy expressions); 1e-12 relative otherwise (an fp64 sum in another order).

Worst measured difference: see ``test_grid_matches_host``."""
import numpy as np
import pytest
import torch

from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
MAP_TOL, MS_TOL, NRMSE_RTOL = 1e-10, 1e-9, 1e-12
TH, TW = 16, 32   # DF.MSMETRIC_TILE (asserted below: the shapes here are aimed at these edges)
# cropped sizes.  MS-SSIM tiles map positions (size - 10): one map position (every level's blur halo is the clamp border only); one row; a
# ragged small one; 40 x 37; one short of / one past a tile edge in each direction; two tile rows exactly
MS_SHAPES = [(11, 11), (11, 50), (12, 37), (40, 37), (TH + 9, TW + 11), (TH + 11, TW + 9), (2 * TH + 10, TW + 10)]
# MATLAB SSIM tiles output pixels: smaller than the halo; one short of / one past a tile edge in each direction; two tile rows exactly
ML_SHAPES = [(1, 1), (1, 7), (5, 5), (TH - 1, TW + 1), (TH + 1, TW - 1), (2 * TH, TW)]
SHAPES = MS_SHAPES + ML_SHAPES


def _cases():
    """every shape with all four (test_y_channel, image_range) pairs, B / C / crop_border rotating as in tests/test_gpu_metrics.py"""
    out = []
    for i, (hc, wc) in enumerate(SHAPES):
        for y in (False, True):
            for rng in (255, 1):
                r = int(rng == 1)
                out.append(dict(hc=hc, wc=wc, B=(1, 3)[(i + y) % 2], C=(3, 1)[(i + r + (i // 2) * y) % 2], crop=(0, 3)[(i + y + r) % 2], y=y, rng=rng,
                                ms=min(hc, wc) >= 11))
    return out


CASES = _cases()
_id = lambda c: f"{c['hc']}x{c['wc']}-B{c['B']}C{c['C']}-cb{c['crop']}-y{int(c['y'])}-r{c['rng']}"  # noqa: E731
WORST = dict(level=0.0, msssim=0.0, matlab=0.0, nrmse=0.0)


def test_case_grid_covers_every_axis():
    from dcpt_amd import functional as DF

    assert DF.MSMETRIC_TILE == (TH, TW) and DF.MSSSIM_MAX_LEVELS == 8
    for sub in (CASES, [c for c in CASES if c["ms"]], [c for c in CASES if not c["ms"]]):
        for k, vals in dict(B=(1, 3), C=(1, 3), crop=(0, 3), y=(False, True), rng=(255, 1)).items():
            assert {c[k] for c in sub} == set(vals), k
    # (the larger MATLAB shapes hold an 11 x 11 window too and go through MS-SSIM as well)
    assert {(c["hc"], c["wc"]) for c in CASES if c["ms"]} == set(MS_SHAPES + ML_SHAPES[3:]) and {(c["hc"], c["wc"]) for c in CASES} == set(SHAPES)
    for rng in (255, 1):
        ms = [c for c in CASES if c["ms"] and c["rng"] == rng]
        assert any(c["y"] and c["C"] == 3 for c in ms) and any(c["y"] and c["C"] == 1 for c in ms) and any(not c["y"] and c["C"] == 3 for c in ms)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _pair(tag, shape):
    """keyed uniform image + bounded noise clipped to [0, 1] (the recipe of tests/test_gpu_metrics.py::_pair)"""
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


def _host_levels(a, b, crop, y, rng, levels):
    """the per-evaluation (SSIM, CS) map means of the host form, (B, levels, 2)"""
    import basicsr.metrics as M

    out = []
    for x, z in M._images(a, b, crop, "BCHW", y, rng):
        per = []
        for k in range(levels):
            per.append(M._ssim_cs(x[..., k % x.shape[2]], z[..., k % x.shape[2]], rng))
            x, z = M._box_blur(x), M._box_blur(z)
        out.append(per)
    return np.array(out, dtype=np.float64)


def _dev(a, b, dev):
    return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)


def _check_msssim(tag, a, b, crop, y, rng, weights, dev, final=True):
    from basicsr.metrics import MSSSIM_WEIGHTS, calculate_msssim, calculate_msssim_device
    from dcpt_amd import functional as DF

    L = len(MSSSIM_WEIGHTS if weights is None else weights)
    ta, tb = _dev(a, b, dev)
    hc, wc = a.shape[2] - 2 * crop, a.shape[3] - 2 * crop
    host = _host_levels(a, b, crop, y, rng, L)
    sums = DF.msssim_sums(ta, tb, crop, y, rng, levels=L)
    assert tuple(sums.shape) == (a.shape[0], L, 2) and sums.dtype == torch.float64
    dl = float(np.abs(sums.cpu().numpy() / ((hc - 10) * (wc - 10)) - host).max())
    WORST["level"] = max(WORST["level"], dl)
    print(f"msssim {tag} L={L}: worst per-level mean |d| {dl:.3e} (1e-10); smallest host mean {host.min():.4f}")
    assert dl <= MAP_TOL, (tag, dl)
    if final:
        assert host.min() >= 0.5, (tag, host.min())   # the premise of the 1e-9 bound
        hv, dv = calculate_msssim(a, b, crop, weights, rng, test_y_channel=y), calculate_msssim_device(ta, tb, crop, weights, rng, test_y_channel=y)
        WORST["msssim"] = max(WORST["msssim"], abs(hv - dv))
        print(f"msssim {tag} L={L}: host {hv!r} device {dv!r} |d| {abs(hv - dv):.3e} (1e-9)")
        assert abs(hv - dv) <= MS_TOL, (tag, hv, dv)


def _check_matlab(tag, a, b, crop, y, rng, dev):
    from basicsr.metrics import calculate_ssim_matlab, calculate_ssim_matlab_device

    hv, dv = calculate_ssim_matlab(a, b, crop, test_y_channel=y, image_range=rng), calculate_ssim_matlab_device(*_dev(a, b, dev), crop, test_y_channel=y, image_range=rng)
    WORST["matlab"] = max(WORST["matlab"], abs(hv - dv))
    print(f"ssim_matlab {tag}: host {hv!r} device {dv!r} |d| {abs(hv - dv):.3e} (1e-10)")
    assert abs(hv - dv) <= MAP_TOL, (tag, hv, dv)


def _check_nrmse(tag, a, b, crop, y, rng, dev):
    from basicsr.metrics import calculate_nrmse, calculate_nrmse_device

    hv, dv = calculate_nrmse(a, b, crop, test_y_channel=y, image_range=rng), calculate_nrmse_device(*_dev(a, b, dev), crop, test_y_channel=y, image_range=rng)
    exact = rng == 255 and not (y and a.shape[1] == 3)
    d = 0.0 if hv == dv else abs(hv - dv) / abs(hv)
    WORST["nrmse"] = max(WORST["nrmse"], d)
    print(f"nrmse {tag}: host {hv!r} device {dv!r} relative |d| {d:.3e} ({'==' if exact else '1e-12'})")
    if exact:
        assert dv == hv, (tag, hv, dv)
    else:
        assert d <= NRMSE_RTOL, (tag, hv, dv)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_grid_matches_host(case, dev):
    """the three device metrics against the host functions on the same fp32 arrays.  Worst differences measured on the MI355X over this
    grid: per-level mean 3.3e-16, MS-SSIM 2.2e-16, MATLAB SSIM 2.2e-16, NRMSE 0 on the exact path and 1.6e-16 relative elsewhere (each
    case prints its figures before it asserts; the running worst is printed with them)."""
    crop, y, rng = case["crop"], case["y"], case["rng"]
    H, W = case["hc"] + 2 * crop, case["wc"] + 2 * crop
    a, b = _pair(f"gpumsm.{case['hc']}x{case['wc']}", (case["B"], case["C"], H, W))
    if case["ms"]:
        _check_msssim(_id(case), a, b, crop, y, rng, None, dev)
    _check_matlab(_id(case), a, b, crop, y, rng, dev)
    _check_nrmse(_id(case), a, b, crop, y, rng, dev)
    print("worst so far:", WORST)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("L", [1, 2, 5, 8])
def test_levels(L, C, dev):
    """weights of every length class on C = 3 without luma (the channel rotation k mod 3) and C = 1; ragged in both directions"""
    a, b = _pair(f"gpumsm.levels{C}", (2, C, TH + 11 + 6, TW + 13 + 6))
    w = {1: [1.0], 2: [0.5, 0.5], 5: None, 8: [0.125] * 8}[L]
    _check_msssim(f"levels-C{C}", a, b, 3, False, 255, w, dev)
    _check_msssim(f"levels-C{C}-r1", a, b, 3, False, 1, w, dev)


def test_nine_levels_raise(dev):
    from basicsr.metrics import calculate_msssim_device
    from dcpt_amd import _lib

    a, b = _dev(*_pair("gpumsm.nine", (1, 3, 24, 24)), dev)
    with pytest.raises(_lib.DcptHipError, match="levels must be 1 .. 8"):
        calculate_msssim_device(a, b, 0, weights=[1.0 / 9] * 9)


@pytest.mark.parametrize("y", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_tie_image_rounds_half_to_even(C, y, dev):
    """the front end in its new uses.  The two tie images are unrelated (their per-level means are ~0.3, under the 0.5 the 1e-9 bound on the
    MS-SSIM product presupposes): the per-level means carry the check, at their own tolerance, and NRMSE its own"""
    a, b = _tie_pair((1, C, 40, 37))
    q = a.astype(np.float32) * np.float32(255.0)
    assert int((q == np.floor(q) + 0.5).sum()) > 100, "the tie image has no ties in fp32: the rounding mode would not matter"
    _check_msssim(f"tie-C{C}-y{int(y)}", a, b, 0, y, 255, None, dev, final=False)
    _check_matlab(f"tie-C{C}-y{int(y)}", a, b, 0, y, 255, dev)
    _check_nrmse(f"tie-C{C}-y{int(y)}", a, b, 0, y, 255, dev)


def _bits(t):
    return t.view(torch.int64)


def _all_three(a, b, crop, y, rng):
    from dcpt_amd import functional as DF

    return [DF.msssim_sums(a, b, crop, y, rng, levels=8), DF.ssim_matlab_sums(a, b, crop, y, rng), DF.image_range_minmax(a, crop, y, rng)]


def test_two_calls_give_identical_bits_and_noncontiguous_inputs_are_taken(dev):
    a, b = _dev(*_pair("gpumsm.bits", (3, 3, 2 * TH + 13, 2 * TW + 13)), dev)
    for y, rng in ((False, 255), (True, 255), (False, 1)):
        r1, r2 = _all_three(a, b, 1, y, rng), _all_three(a, b, 1, y, rng)
        assert [tuple(t.shape) for t in r1] == [(3, 8, 2), (3, 1 if y else 3), (3, 2)] and all(t.dtype == torch.float64 for t in r1)
        # a channels_last view / a sliced view of a larger tensor: .contiguous() inside, the same bits out
        r3 = _all_three(a.contiguous(memory_format=torch.channels_last), torch.cat([b, b], 3)[..., : b.shape[3]], 1, y, rng)
        for t1, t2, t3 in zip(r1, r2, r3):
            assert torch.equal(_bits(t1), _bits(t2)) and torch.equal(_bits(t1), _bits(t3))
    # the range against torch on the quantised values
    q = (a[:, :, 1:-1, 1:-1] * 255.0).round()
    mm = _all_three(a, b, 1, False, 255)[2]
    assert torch.equal(mm[:, 0], q.amin(dim=(1, 2, 3)).double()) and torch.equal(mm[:, 1], q.amax(dim=(1, 2, 3)).double())


def test_accumulator_matches_single_calls(dev):
    """MetricSums over three batches of different shapes: one transfer at the end, the per-batch values of the single-call functions"""
    from basicsr.metrics import (MetricSums, calculate_msssim_device, calculate_nrmse_device, calculate_psnr_device, calculate_ssim_device,
                                 calculate_ssim_matlab_device)

    w = [0.2, 0.3, 0.5]
    acc = MetricSums(crop_border=3, test_y_channel=True, msssim=True, weights=w, ssim_matlab=True, nrmse=True)
    only = MetricSums(crop_border=3, test_y_channel=True, psnr=False, ssim=False, nrmse=True)
    pairs = []
    for k, shape in enumerate([(1, 3, 30, 41), (2, 3, 17, 64), (1, 1, 48, 48)]):
        pairs.append(_dev(*_pair(f"gpumsm.acc{k}", shape), dev))
        acc.add(*pairs[-1])
        only.add(*pairs[-1])
    res = acc.result()
    assert list(res) == ["psnr", "ssim", "msssim", "ssim_matlab", "nrmse"]
    assert res["psnr"] == [calculate_psnr_device(a, b, 3, test_y_channel=True) for a, b in pairs]
    assert res["ssim"] == [calculate_ssim_device(a, b, 3, test_y_channel=True) for a, b in pairs]
    assert res["msssim"] == [calculate_msssim_device(a, b, 3, weights=w, test_y_channel=True) for a, b in pairs]
    assert res["ssim_matlab"] == [calculate_ssim_matlab_device(a, b, 3, test_y_channel=True) for a, b in pairs]
    assert res["nrmse"] == [calculate_nrmse_device(a, b, 3, test_y_channel=True) for a, b in pairs]
    assert only.result() == {"psnr": [], "ssim": [], "nrmse": res["nrmse"]}
    # the defaults: today's keys and today's words (sse, then the SSIM sums, per add)
    a, b = pairs[1]
    old = MetricSums(crop_border=3)
    old.add(a, b)
    assert list(old.result()) == ["psnr", "ssim"] and [t.numel() for t in old.pending()] == [2, 6]
    # inf and the batch of identical images share the host's semantics
    assert calculate_nrmse_device(a, torch.cat([b[:1], a[1:]]), 3) == float("inf")
    assert abs(calculate_msssim_device(a, a.clone(), 3) - 1.0) <= 1e-12 and abs(calculate_ssim_matlab_device(a, a.clone(), 3) - 1.0) <= 1e-12


def test_stays_inside_its_buffers(dev):
    from redzone import redzone

    a, b = _dev(*_pair("gpumsm.rz", (3, 3, TH + 11 + 6, TW + 9 + 6)), dev)
    ref = [_all_three(a, b, 3, y, rng) for y, rng in ((False, 255), (True, 1))]
    with redzone() as rz:
        got = [_all_three(a, b, 3, y, rng) for y, rng in ((False, 255), (True, 1))]
    assert rz.count > 0
    for r, g in zip(ref, got):   # (a workspace that starts as NaNs: nothing unwritten is read)
        for t0, t1 in zip(r, g):
            assert torch.equal(_bits(t0), _bits(t1))


def test_launch_trace_names_the_new_kernels(dev):
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    a, b = _dev(*_pair("gpumsm.trace", (1, 3, 24, 24)), dev)
    with kernel_trace() as t:
        _all_three(a, b, 0, False, 255)
    t.assert_ran("metric.ms_level", "metric.ms_reduce", "metric.matlab_tile", "metric.matlab_reduce", "metric.range_tile", "metric.range_reduce")
    assert set(t.families()) == set(t.families("metric.")) and sum(t.counts.values()) == 6
    with kernel_trace() as t:   # dcpt_imgmetric keeps its three tags
        DF.image_metric_sums(a, b)
        DF.image_metric_sums(a, b, ssim=False)
    assert set(t.counts) == {"metric.tile_ssim", "metric.tile_psnr", "metric.reduce"} and t["metric.reduce"] == 2


def test_bad_arguments_raise(dev):
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    a = torch.rand(1, 3, 16, 16, device=dev)
    three = (lambda x, c: DF.msssim_sums(x, x, c), lambda x, c: DF.ssim_matlab_sums(x, x, c), lambda x, c: DF.image_range_minmax(x, c))
    for f in three:
        with pytest.raises(_lib.DcptHipError, match="C must be 1 or 3"):
            f(a[:, :2], 0)
        with pytest.raises(_lib.DcptHipError, match="crop_border must be >= 0"):
            f(a, -1)
        with pytest.raises(_lib.DcptHipError, match="nothing left after the crop"):
            f(a, 8)
        with pytest.raises(_lib.DcptHipError):
            f(a.cpu(), 0)
    with pytest.raises(_lib.DcptHipError, match="at least 11 x 11"):
        DF.msssim_sums(a, a, 3)
    for levels in (0, 9):
        with pytest.raises(_lib.DcptHipError, match="levels must be 1 .. 8"):
            DF.msssim_sums(a, a, 0, levels=levels)
    with pytest.raises(_lib.DcptHipError, match="above 65535"):
        DF.msssim_sums(a.expand(2731, 3, 16, 16), a.expand(2731, 3, 16, 16), 0, levels=8)   # 2731 * 3 * 8 = 65544
    with pytest.raises(ValueError):
        DF.msssim_sums(a, a, image_range=65535)
    with pytest.raises(ValueError):
        DF.ssim_matlab_sums(a, a[..., :8])
    # a workspace that is too small, straight at the C ABI (real pointers: the check comes before any launch)
    out = torch.empty(1, 5, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(1 << 12, dtype=torch.uint8, device=dev)
    for rc in (lib.dcpt_msssim(a.data_ptr(), a.data_ptr(), out.data_ptr(), ws.data_ptr(), 8, 1, 3, 16, 16, 0, 0, 5, None),
               lib.dcpt_ssim_matlab(a.data_ptr(), a.data_ptr(), out.data_ptr(), ws.data_ptr(), 8, 1, 3, 16, 16, 0, 0, None),
               lib.dcpt_imgrange(a.data_ptr(), out.data_ptr(), ws.data_ptr(), 8, 1, 3, 16, 16, 0, 0, None)):
        assert rc != 0 and b"workspace too small" in lib.dcpt_last_error()


# ---- SRModel.nondist_validation -------------------------------------------------------------------------------------------------------
TINY = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1])
METRICS = dict(msssim=dict(type="calculate_msssim", crop_border=2, test_y_channel=True),
               ssim_matlab=dict(type="calculate_ssim_matlab", crop_border=0, test_y_channel=False),
               nrmse=dict(type="calculate_nrmse", crop_border=0, test_y_channel=False),
               psnr=dict(type="calculate_psnr", crop_border=0, test_y_channel=False))


def _validate(device_metrics, metrics=None):
    from basicsr.data import build_dataloader, build_dataset
    from basicsr.models import build_model
    from dcpt_amd.keyed_init import fill_module_

    val = dict(save_img=False, metrics=metrics or METRICS)
    if device_metrics is not None:
        val["device_metrics"] = device_metrics
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="NAFNetBaseline", window_size=16, **TINY), path=dict(pretrain_network_g=None, visualization=None), val=val)
    m = build_model(opt)
    fill_module_(m.net_g)
    dopt = dict(name="syn", type="SyntheticPairedDataset", phase="val", num=2, size=(40, 37), seed=3)
    return m, build_dataloader(build_dataset(dopt), dopt)


def _close(h, d, tol):
    return (np.isnan(h) and np.isnan(d)) or h == d or abs(h - d) <= tol


def test_validation_device_route_matches_host_route(dev, monkeypatch):
    from basicsr.models.sr_model import SRModel

    m0, loader = _validate(None)
    host = dict(m0.nondist_validation(loader, 1, None, False))
    m1, loader = _validate(True)
    plan = m1._device_metric_plan(METRICS, True)
    assert plan == {"msssim": (("msssim", 2, True, 255, None), "msssim"), "ssim_matlab": (("ssim_matlab", 0, False, 255), "ssim_matlab"),
                    "nrmse": (("nrmse", 0, False, 255), "nrmse"), "psnr": ((0, False, 255), "psnr")}
    calls = []
    monkeypatch.setattr(SRModel, "get_current_visuals", lambda self: calls.append(1) or (_ for _ in ()).throw(AssertionError("get_current_visuals called")))
    got = dict(m1.nondist_validation(loader, 1, None, False))
    print(f"validation: host {host} device {got}")
    assert not calls and list(got) == list(host) and m1.metric_results == got
    assert got["psnr"] == host["psnr"] and got["nrmse"] == host["nrmse"] and np.isfinite(host["nrmse"])
    assert _close(host["ssim_matlab"], got["ssim_matlab"], MAP_TOL) and _close(host["msssim"], got["msssim"], MS_TOL)
    # the key carries the weights; nine of them, another order or another range stay on the host
    more = dict(a=dict(type="calculate_msssim", crop_border=0, weights=[0.5, 0.5]), b=dict(type="calculate_msssim", crop_border=0, weights=[1 / 9] * 9),
                c=dict(type="calculate_nrmse", crop_border=0, input_order="BHWC"), d=dict(type="calculate_ssim_matlab", crop_border=0, image_range=65535),
                e=dict(type="calculate_psnr_pt", crop_border=0))
    assert m1._device_metric_plan(more, True) == {"a": (("msssim", 0, False, 255, (0.5, 0.5)), "msssim")}


def test_validation_without_clamp_stays_on_the_host(dev, monkeypatch):
    from dcpt_amd import functional as DF

    m0, loader = _validate(None)
    host = dict(m0.nondist_validation(loader, 1, None, False, clamp=False))
    m1, loader = _validate(True)
    assert m1._device_metric_plan(METRICS, False) == {}
    for name in ("image_metric_sums", "msssim_sums", "ssim_matlab_sums", "image_range_minmax"):
        monkeypatch.setattr(DF, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("device metrics without clamp")))
    got = dict(m1.nondist_validation(loader, 1, None, False, clamp=False))
    assert list(got) == list(host) and all(_close(host[k], got[k], 0.0) for k in host)
