"""CPU: the host NIQE (basicsr.metrics.calculate_niqe) and the host ``imresize`` (basicsr.utils.imresize) against the reference's own
outputs (tests/golden/niqe.npz, imresize.npz, made by tools/make_golden_niqe.py), plus refusals and plumbing.

The bounds are multiples of what the tool measured between the kernel-blind float64 restatement (tests/niqe_restatement.py) and the
reference's float32 pipeline -- the spread is the reference's own rounding -- never of what the code under test gives:

  imresize   largest |restatement - reference| over the 11 fixture cases 1.211e-07 (per case 6.2e-08 .. 1.2e-07); allowed 4 x that
  scores     relative deviation (a) 9.338e-07, (b) 8.750e-07, (c) 2.768e-06; allowed 8 x the largest
  features   other than alpha: largest relative deviation (a) 3.583e-05, (b) 7.538e-05, (c) 3.956e-05; allowed 8 x the largest
  alpha      lives on a 0.001 grid: at most 1 % of the entries may sit one step from the reference's, none further (the restatement's own
             count on these images: 0 of 40, 0 of 180, 0 of 60)

Case (d) (crop_border 4 on a 1 x 3 image) is a documented departure: the reference slices the plane axis and returns NaN; here the crop
is spatial and the result equals the restatement on the cropped planes."""
import os

import numpy as np
import pytest
import torch

import niqe_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRIS = os.path.join(GOLDEN, "niqe_pris_params.npz")
RESIZE_TOL = 4 * 1.211e-07
SCORE_RTOL = 8 * 2.768e-06
FEATURE_RTOL = 8 * 7.538e-05
ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
RESIZE_CASES = ["8x8_s2", "13x9_s2", "24x20_s2", "8x8_s2_noaa", "13x9_s2_noaa", "24x20_s2_noaa", "13x9_s3", "24x20_s3", "24x20_s4", "5x7_x2",
                "5x7_x4"]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "niqe.npz")) as f:
        d = {k: f[k] for k in f.files}
    for tag in "abc":
        d[f"{tag}.img"] = R.decode_planes(d[f"{tag}.planes_dx"]).astype(np.float32) / np.float32(255.0)
        d[f"{tag}.scale2"] = R.decode_f32(d[f"{tag}.scale2_bytes"])
    return d


@pytest.fixture(scope="module")
def resize_gold():
    with np.load(os.path.join(GOLDEN, "imresize.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def pris():
    with np.load(PRIS) as f:
        return f["mu_pris_param"].astype(np.float64), f["cov_pris_param"].astype(np.float64)


# ---- imresize ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", RESIZE_CASES)
def test_host_imresize_matches_reference(resize_gold, tag):
    from basicsr.utils import imresize

    g = resize_gold
    h, w = (int(v) for v in g[f"{tag}.size"])
    x, scale, aa = g[f"x.{h}x{w}"], float(g[f"{tag}.scale"]), bool(g[f"{tag}.antialiasing"])
    y_np = imresize(x, scale, antialiasing=aa)
    y_t = imresize(torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))), scale, antialiasing=aa)
    assert y_np.dtype == np.float32 and y_np.shape == g[f"{tag}.y_hwc"].shape
    assert y_t.dtype == torch.float32 and tuple(y_t.shape) == g[f"{tag}.y_chw"].shape
    e_np = float(np.abs(y_np.astype(np.float64) - g[f"{tag}.y_hwc"]).max())
    e_t = float(np.abs(y_t.numpy().astype(np.float64) - g[f"{tag}.y_chw"]).max())
    print(f"imresize {tag}: numpy HWC {e_np:.3e}, tensor CHW {e_t:.3e} (bound {RESIZE_TOL:.3e})")
    assert e_np <= RESIZE_TOL and e_t <= RESIZE_TOL
    # a 2-D input keeps its rank in both conventions
    assert np.array_equal(imresize(x[..., 0], scale, antialiasing=aa), y_np[..., 0])
    assert torch.equal(imresize(torch.from_numpy(x[..., 0].copy()), scale, antialiasing=aa), y_t[0])


def test_host_imresize_tables_restate_the_reference(resize_gold):
    """rows sum to 1, the first taps are the reference's ``left`` and a restated table gives the restatement's output to float64 rounding"""
    from dcpt_amd.matlab_resize import resize_planes, weights_indices

    for n, scale, aa in ((24, 0.5, True), (13, 1 / 3, True), (20, 0.25, True), (7, 2, True), (9, 0.5, False)):
        first, weights = weights_indices(n, scale, aa)
        idx, wr = R.weights_indices(n, len(first), scale, aa, np.float64)
        assert np.array_equal(first, idx[:, 0] - 1) and np.abs(weights - wr).max() <= 1e-15 and np.abs(weights.sum(1) - 1).max() <= 1e-15
    x = resize_gold["x.24x20"].transpose(2, 0, 1)
    assert np.abs(resize_planes(x, 1 / 3, True) - R.imresize_planes(x, 1 / 3, True, np.float64)).max() <= 1e-15


def test_too_short_input_is_refused():
    from basicsr.utils import imresize

    with pytest.raises(ValueError, match="shorter than the kernel reaches"):
        imresize(np.zeros((3, 3, 1), dtype=np.float32), 0.25)          # 16-wide kernel on three pixels
    with pytest.raises(ValueError, match="shorter than the kernel reaches"):
        imresize(torch.zeros(1, 40, 2), 0.5)
    assert imresize(np.zeros((8, 8), dtype=np.float32), 0.5).shape == (4, 4)   # every tap reflects, none leaves


# ---- NIQE ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_host_niqe_matches_reference(gold, pris, tag):
    from basicsr.metrics import calculate_niqe
    from basicsr.metrics.niqe import features_from_stats, niqe_block_stats

    img, ref = gold[f"{tag}.img"], float(gold[f"{tag}.score"])
    got = calculate_niqe(img, 0, pris_params=PRIS)
    rel = abs(got - ref) / abs(ref)
    rows, ref_rows = features_from_stats(niqe_block_stats(img, 0)), gold[f"{tag}.distparam"]
    assert rows.shape == ref_rows.shape
    assert np.array_equal(np.isnan(rows), np.isnan(ref_rows)), "NaN positions differ from the reference's"
    da = np.abs(rows[..., ALPHA_COLS] - ref_rows[..., ALPHA_COLS])
    steps = int((da > 5e-4).sum())
    other = np.setdiff1d(np.arange(36), ALPHA_COLS)
    x, y = rows[..., other], ref_rows[..., other]
    ok = ~np.isnan(y)
    frel = float((np.abs(x[ok] - y[ok]) / np.abs(y[ok])).max())
    print(f"niqe {tag}: {got:.9f} against {ref:.9f}, relative {rel:.3e} (bound {SCORE_RTOL:.3e}); alpha one step apart {steps} of {da.size}; "
          f"other features {frel:.3e} (bound {FEATURE_RTOL:.3e})")
    assert rel <= SCORE_RTOL
    assert not (da > 1.5e-3).any() and steps <= 0.01 * da.size
    assert frel <= FEATURE_RTOL
    # the scale-2 image against the reference's float32 resize (its values are in [0, 1]: the imresize bound applies)
    _, parts = niqe_block_stats(img, 0, parts=True)
    assert np.abs(parts["img2"] - gold[f"{tag}.scale2"]).max() <= RESIZE_TOL


def test_flat_block_has_the_references_nan_pattern(gold, pris):
    """case (c): the first block is exactly zero at both scales: 13 NaN of 18 per scale, alpha = 0.2, and the score is finite"""
    from basicsr.metrics import calculate_niqe
    from basicsr.metrics.niqe import features_from_stats, niqe_block_stats

    stats, parts = niqe_block_stats(gold["c.img"], 0, parts=True)
    assert not parts["mscn1"][0, :96, :96].any() and not parts["mscn2"][0, :48, :48].any()
    assert not stats[0, 0, :, :, :].any()   # counts and sums exactly zero
    rows, ref_rows = features_from_stats(stats), gold["c.distparam"]
    nan = np.isnan(rows[0, 0])
    assert np.array_equal(nan, np.isnan(ref_rows[0, 0])) and nan.sum() == 26 and nan[:18].sum() == 13
    assert np.all(rows[0, 0, ALPHA_COLS] == 0.2) and not np.isnan(rows[0, 1:]).any()
    assert np.isfinite(calculate_niqe(gold["c.img"], 0, pris_params=PRIS))


def test_crop_border_crops_the_planes(gold, pris):
    """case (d): the reference returns NaN (its crop slices the plane axis); here the crop is spatial.  Two float64 evaluations of one
    formula in different summation orders: 1e-8 relative leaves room for the conditioning of the 36 x 36 pseudo-inverse"""
    from basicsr.metrics import calculate_niqe

    assert np.isnan(gold["d.score"])
    got = calculate_niqe(gold["b.img"], 4, pris_params=PRIS)
    want = R.niqe(gold["b.img"], 4, *pris)
    print(f"niqe d: {got:.12f} against the restatement's {want:.12f}")
    assert np.isfinite(got) and abs(got - want) <= 1e-8 * abs(want)
    assert abs(got - calculate_niqe(gold["b.img"], 0, pris_params=PRIS)) > 1e-3   # (the crop moves the block grid: another score)


def test_refusals(gold, monkeypatch, tmp_path):
    from basicsr.metrics import calculate_niqe
    from basicsr.metrics import niqe as N

    one_block = np.zeros((1, 1, 191, 96), dtype=np.float32)
    with pytest.raises(ValueError, match="at least two whole"):
        calculate_niqe(one_block, 0, pris_params=PRIS)
    with pytest.raises(ValueError, match="at least two whole"):
        calculate_niqe(gold["a.img"], 1, pris_params=PRIS)             # 190 x 94 after the crop
    with pytest.raises(ValueError, match="BCHW"):
        calculate_niqe(gold["a.img"].transpose(0, 2, 3, 1), 0, input_order="BHWC", pris_params=PRIS)
    with pytest.raises(ValueError, match="B, C, H, W"):
        calculate_niqe(gold["a.img"][0], 0, pris_params=PRIS)
    monkeypatch.delenv("DCPT_NIQE_PRIS_PARAMS", raising=False)
    assert not os.path.exists(os.path.join(os.path.dirname(N.__file__), "niqe_pris_params.npz")), "the pristine model is not committed there"
    with pytest.raises(FileNotFoundError, match="DCPT_NIQE_PRIS_PARAMS"):
        calculate_niqe(gold["a.img"], 0)
    with pytest.raises(FileNotFoundError, match="do not exist"):
        calculate_niqe(gold["a.img"], 0, pris_params=str(tmp_path / "nothing.npz"))
    monkeypatch.setenv("DCPT_NIQE_PRIS_PARAMS", PRIS)
    assert calculate_niqe(gold["a.img"], 0) == calculate_niqe(gold["a.img"], 0, pris_params=PRIS)
    with np.load(PRIS) as f:
        assert calculate_niqe(gold["a.img"], 0, pris_params=dict(f)) == calculate_niqe(gold["a.img"], 0)


def test_registry_and_validation_plumbing(gold):
    from basicsr.metrics import calculate_metric, calculate_niqe
    from basicsr.models.sr_model import SRModel
    from basicsr.utils.registry import METRIC_REGISTRY

    assert METRIC_REGISTRY.get("calculate_niqe") is calculate_niqe and METRIC_REGISTRY.get("calculate_niqe_device") is not None
    img = gold["a.img"]
    opt = dict(type="calculate_niqe", crop_border=0, pris_params=PRIS)
    assert calculate_metric(dict(img=img, img2=img), opt) == calculate_niqe(img, 0, pris_params=PRIS)   # (img2 is accepted and ignored)

    metrics = dict(niqe=dict(type="calculate_niqe", crop_border=2, pris_params=PRIS), psnr=dict(type="calculate_psnr", crop_border=0),
                   niqe_hwc=dict(type="calculate_niqe", crop_border=0, input_order="BHWC"))
    model = SRModel.__new__(SRModel)
    model.device = torch.device("cuda")
    model.opt = dict(val=dict(device_metrics=True))
    assert model._device_metric_plan(metrics, True) == {"niqe": (("niqe", 2, PRIS), "niqe"), "psnr": ((0, False, 255), "psnr")}
    assert model._device_metric_plan(metrics, False) == {}
    model.opt = dict(val=dict())
    assert model._device_metric_plan(metrics, True) == {}


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """the C ABI without a device: the workspace query answers (0 for what the entry point refuses), and null pointers, bad shapes, unknown
    flags and short workspaces are reported before anything is launched (the pointers here are never dereferenced)"""
    from dcpt_amd import _lib

    lib = _lib.load()
    P = 0x1000
    err = lambda: lib.dcpt_last_error().decode()
    geo = (3, 192, 288, 96, 144, 10, 10)
    need = lib.dcpt_imresize_ws_bytes(*geo)
    assert need == 3 * 96 * 288 * 8
    assert lib.dcpt_imresize_ws_bytes(0, 192, 288, 96, 144, 10, 10) == 0 and lib.dcpt_imresize_ws_bytes(3, 192, 288, 96, 144, 0, 10) == 0
    assert lib.dcpt_imresize_ws_bytes(1, 40000, 40000, 20000, 20000, 10, 10) == 0
    rs = lambda x, ws, n, g, ps, rstride, flags: lib.dcpt_imresize_fwd(x, P, P, P, P, P, ws, n, *g, ps, rstride, flags, None)
    assert rs(None, P, need, geo, 192 * 288, 288, 0) != 0 and "null" in err()
    assert rs(P, P, need - 1, geo, 192 * 288, 288, 0) != 0 and "workspace too small" in err()
    assert rs(P, None, need, geo, 192 * 288, 288, 0) != 0 and "workspace too small" in err()
    assert rs(P, P, need, geo, 192 * 288, 288, 8) != 0 and "unknown flags" in err()
    assert rs(P, P, need, geo, 192 * 288, 288, 1 | 4) != 0 and "fp32 source" in err()
    assert rs(P, P, need, geo, 192 * 288, 287, 0) != 0 and "strides" in err()
    assert rs(P, P, need, geo, 191 * 288, 288, 0) != 0 and "strides" in err()
    assert rs(P, P, need, (3, 192, 288, 96, 144, 5000, 10), 192 * 288, 288, 0) != 0 and "tap count" in err()
    mscn, st = lib.dcpt_niqe_mscn_fwd, lib.dcpt_niqe_block_stats_fwd
    assert mscn(None, P, 1, 192, 96, 0, 1, None) != 0 and "null" in err()
    assert mscn(P, P, 1, 192, 96, 0, 3, None) != 0 and "scale must be 1 or 2" in err()
    assert mscn(P, P, 1, 95, 300, 0, 1, None) != 0 and "no whole 96 x 96 block" in err()
    assert mscn(P, P, 1, 200, 300, 60, 1, None) != 0 and "no whole 96 x 96 block" in err()
    assert mscn(P, P, 1, 200, 300, 100, 1, None) != 0 and "nothing left after the crop" in err()
    assert mscn(P, P, 1, 96, 100, 0, 2, None) != 0 and "whole 48 x 48 blocks" in err()
    assert mscn(P, P, 70000, 96, 96, 0, 1, None) != 0 and "65535" in err()
    assert st(P, None, 1, 96, 96, 96, None) != 0 and "null" in err()
    assert st(P, P, 1, 96, 96, 64, None) != 0 and "96 or 48" in err()
    assert st(P, P, 1, 96, 100, 48, None) != 0 and "whole blocks" in err()
