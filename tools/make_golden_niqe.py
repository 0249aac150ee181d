"""Golden vectors of the reference's NIQE and ``imresize`` (build container only; needs the reference tree and scipy).

    python tools/make_golden_niqe.py [REFERENCE_ROOT]

Loads the reference's basicsr/metrics/niqe.py and basicsr/utils/matlab_functions.py by file path under private module names; ``cv2`` is
an empty stub (the live code path never calls it), ``metric_util`` and the registry are stand-ins of a few lines.  Writes

  tests/golden/niqe_pris_params.npz   a copy of the reference's pristine model (data the reference reads)
  tests/golden/imresize.npz           inputs and the reference's outputs: numpy HWC and tensor CHW, scales 0.5, 1/3, 0.25, 2, 4,
                                      antialiasing on and off at 0.5
  tests/golden/niqe.npz               cases (a)-(c): the uint8 planes (as differences along W), the reference's score, its distparam rows and its scale-2 image (as byte planes);
                                      case (d): the reference's score only (NaN: its crop slices the plane axis)

and prints what the tests' bounds are made of: per imresize case the largest deviation of the float64 restatement
(tests/niqe_restatement.py) from the reference's float32 output; per NIQE case the relative deviation of the restatement's score and
features, the count of alpha entries one grid step apart, and per block the share of non-zero longdouble MSCN elements below 1e-9 in magnitude (a
sign the arithmetic may legitimately flip).  Single-threaded CPU, seeded: a rerun reproduces the files."""
from __future__ import annotations

import importlib.util
import os
import shutil
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import niqe_restatement as R  # noqa: E402
from oracle import ref_import  # noqa: E402  (REF: where the reference tree lives)

GOLDEN = os.path.join(ROOT, "tests", "golden")
RESIZE_CASES = [   # (tag, (h, w), scale, antialiasing)
    ("8x8_s2", (8, 8), 0.5, True), ("13x9_s2", (13, 9), 0.5, True), ("24x20_s2", (24, 20), 0.5, True),
    ("8x8_s2_noaa", (8, 8), 0.5, False), ("13x9_s2_noaa", (13, 9), 0.5, False), ("24x20_s2_noaa", (24, 20), 0.5, False),
    ("13x9_s3", (13, 9), 1 / 3, True), ("24x20_s3", (24, 20), 1 / 3, True),
    ("24x20_s4", (24, 20), 0.25, True),
    ("5x7_x2", (5, 7), 2, True), ("5x7_x4", (5, 7), 4, True),
]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref_root):
    """-> (the reference's niqe module, its matlab_functions module), loaded without its package __init__"""
    mine = {k: v for k, v in sys.modules.items() if k == "cv2" or k == "basicsr" or k.startswith("basicsr.")}
    for k in mine:
        del sys.modules[k]
    try:
        for name in ("cv2", "basicsr", "basicsr.metrics", "basicsr.utils", "basicsr.metrics.metric_util", "basicsr.utils.registry"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["basicsr.metrics.metric_util"].reorder_image = sys.modules["basicsr.metrics.metric_util"].to_y_channel = None

        class _Registry:
            def register(self, obj=None):
                return (lambda f: f) if obj is None else obj

        sys.modules["basicsr.utils.registry"].METRIC_REGISTRY = _Registry()
        mf = _load("_ref_matlab_functions", os.path.join(ref_root, "basicsr", "utils", "matlab_functions.py"))
        sys.modules["basicsr.utils.matlab_functions"] = mf
        nq = _load("_ref_niqe", os.path.join(ref_root, "basicsr", "metrics", "niqe.py"))
        return nq, mf
    finally:
        for k in [k for k in sys.modules if k == "cv2" or k == "basicsr" or k.startswith("basicsr.")]:
            del sys.modules[k]
        sys.modules.update(mine)


def make_plane(rng, h, w):
    """an 8-bit plane with image-like statistics: a smooth field plus fine texture (white noise alone has no structure for the AGGD fit)"""
    from scipy.ndimage import zoom

    base = zoom(rng.uniform(100, 150, (h // 16 + 2, w // 16 + 2)), 16, order=3)[:h, :w]
    mid = zoom(rng.normal(0, 5, (h // 4 + 2, w // 4 + 2)), 4, order=3)[:h, :w]
    return np.clip(np.rint(base + mid + rng.normal(0, 1.5, (h, w))), 0, 255).astype(np.uint8)


def gen_imresize(mf):
    rng = np.random.default_rng(20260)
    out, worst, inputs = {}, 0.0, {}
    for tag, (h, w), scale, aa in RESIZE_CASES:
        if (h, w) not in inputs:   # one input per size, shared by its cases
            inputs[(h, w)] = out[f"x.{h}x{w}"] = rng.random((h, w, 3), dtype=np.float32)
        x = inputs[(h, w)]
        y_np = mf.imresize(x, scale, antialiasing=aa)
        y_t = mf.imresize(torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))), scale, antialiasing=aa).numpy()
        assert np.array_equal(y_np.transpose(2, 0, 1), y_t), tag
        r64 = R.imresize_planes(x.transpose(2, 0, 1), scale, aa, np.float64)
        dev = float(np.abs(r64 - y_t).max())
        worst = max(worst, dev)
        print(f"imresize {tag}: {h} x {w} -> {y_t.shape[1]} x {y_t.shape[2]}, float64 restatement against the reference's fp32 output {dev:.3e}")
        out[f"{tag}.y_hwc"], out[f"{tag}.y_chw"] = y_np, y_t
        out[f"{tag}.size"], out[f"{tag}.scale"], out[f"{tag}.antialiasing"] = np.array([h, w]), np.float64(scale), np.bool_(aa)
    print(f"imresize: largest deviation {worst:.3e}")
    out["max_dev"] = np.float64(worst)
    np.savez_compressed(os.path.join(GOLDEN, "imresize.npz"), **out)


def run_reference(nq, img01, crop_border, single_plane=False):
    """the reference's score, its distparam rows [P][nblk][36] and its scale-2 images [P][h/2][w/2] (float32, in [0, 1])"""
    feats, scale2 = [], []
    orig_cf, orig_rs = nq.compute_feature, nq.imresize

    def cf(block):
        f = orig_cf(block)
        feats.append(f)
        return f

    def rs(img, **kw):
        y = orig_rs(img, **kw)
        scale2.append(np.array(y))
        return y

    nq.compute_feature, nq.imresize = cf, rs
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if single_plane:   # the reference's wrapper iterates over the rows of a lone plane and asserts: its inner function is called
                pris = np.load(os.path.join(os.path.dirname(nq.__file__), "niqe_pris_params.npz"))
                plane = (img01[0, 0].astype(np.float32) * 255.0).round()
                score = nq.niqe(plane, pris["mu_pris_param"], pris["cov_pris_param"], pris["gaussian_window"])
            else:
                score = float(nq.calculate_niqe(img01, crop_border))
    finally:
        nq.compute_feature, nq.imresize = orig_cf, orig_rs
    p = len(scale2)
    if p == 0:
        return score, None, None
    per = len(feats) // p
    rows = [np.concatenate([np.array(feats[i * per:i * per + per // 2]), np.array(feats[i * per + per // 2:(i + 1) * per])], axis=1) for i in range(p)]
    return score, np.array(rows), np.array(scale2)


def report(tag, img01, crop, ref_score, ref_rows, mu, cov):
    parts64, partsT = R.pipeline(img01, crop, np.float64), R.pipeline(img01, crop, np.longdouble)
    rows = R.features(parts64)
    s = float(np.mean([R.score(r, mu, cov) for r in rows]))
    line = f"niqe {tag}: restatement {s:.9f}"
    if ref_rows is not None:
        line += f", reference {ref_score:.9f}, relative deviation {abs(s - ref_score) / abs(ref_score):.3e}"
        assert np.array_equal(np.isnan(rows), np.isnan(ref_rows)), f"{tag}: NaN pattern differs from the reference"
        alpha_cols = [0] + [2 + 4 * k for k in range(4)] + [18] + [20 + 4 * k for k in range(4)]
        a, b = rows[..., alpha_cols], ref_rows[..., alpha_cols]
        step = np.abs(a - b) > 5e-4
        assert not (np.abs(a - b) > 1.5e-3).any(), f"{tag}: an alpha more than one grid step apart"
        other = np.ones(36, dtype=bool)
        other[alpha_cols] = False
        x, y = rows[..., other], ref_rows[..., other]
        ok = ~np.isnan(y)
        rel = float((np.abs(x[ok] - y[ok]) / np.abs(y[ok])).max())
        line += f"; alpha one step apart {int(step.sum())} of {step.size} ({100.0 * step.mean():.2f} %, cap 1 %); other features {rel:.3e}"
        if step.any():   # (the cap of the tests is 1 %; the fixture keeps to images without any, so the other features' bound stays tight)
            print(line)
            raise ContestedAlpha(f"{tag}: {int(step.sum())} alpha entries one grid step from the reference's")
    print(line)
    for key, bs in (("mscn1", 96), ("mscn2", 48)):
        worst = 0.0
        for plane in partsT[key]:
            for _, maps in R.block_maps(plane, bs):
                worst = max(worst, max(float(((np.abs(m) < 1e-9) & (m != 0)).mean()) for m in maps))
        zero_blocks = sum(int(not np.any(maps[0])) for plane in partsT[key] for _, maps in R.block_maps(plane, bs))
        print(f"    {key}: largest share of 0 < |T| < 1e-9 per block map {100.0 * worst:.3f} % (cap 0.1 %); {zero_blocks} exactly-zero blocks")
    return s


class ContestedAlpha(Exception):
    pass


def _niqe_cases(nq, rng, mu, cov):
    a = np.stack([make_plane(rng, 192, 96) for _ in range(2)])[:, None]
    b = np.stack([make_plane(rng, 200, 300) for _ in range(3)])[None]
    c = b[:, :1].copy()
    c[0, 0, :112, :112] = 117
    out = {}
    for tag, planes, crop, single in (("a", a, 0, False), ("b", b, 0, False), ("c", c, 0, True), ("d", b, 4, False)):
        img01 = planes.astype(np.float32) / np.float32(255.0)
        assert np.array_equal((img01 * 255.0).round(), planes.astype(np.float32))
        try:
            score, rows, scale2 = run_reference(nq, img01, crop, single)
        except Exception as e:   # (d): the reference's crop may also leave nothing whole
            score, rows, scale2 = float("nan"), None, None
            print(f"niqe {tag}: the reference raised {type(e).__name__}: {e}")
        if tag == "d":
            print(f"niqe d: the reference returns {score} (its crop slices the plane axis and H)")
            report(tag, img01, crop, score, None, mu, cov)
            out["d.score"] = np.float64(score)
            continue
        if tag == "c":
            nan_per_row = np.isnan(rows[0, 0]).sum()
            print(f"niqe c: the first block's row holds {int(nan_per_row)} NaN of 36")
        report(tag, img01, crop, score, rows, mu, cov)
        assert np.array_equal(R.decode_planes(R.encode_planes(planes)), planes) and np.array_equal(R.decode_f32(R.encode_f32(scale2)), scale2)
        out[f"{tag}.planes_dx"], out[f"{tag}.scale2_bytes"] = R.encode_planes(planes), R.encode_f32(scale2)   # (niqe_restatement's codecs)
        out[f"{tag}.score"], out[f"{tag}.distparam"] = np.float64(score), rows
    return out


def gen_niqe(nq):
    shutil.copyfile(os.path.join(os.path.dirname(nq.__file__), "niqe_pris_params.npz"), os.path.join(GOLDEN, "niqe_pris_params.npz"))
    pris = np.load(os.path.join(GOLDEN, "niqe_pris_params.npz"))
    mu, cov = pris["mu_pris_param"], pris["cov_pris_param"]
    g = R.window(np.float64)
    print(f"gaussian window: computed against stored {float(np.abs(g - pris['gaussian_window']).max()):.2e}")
    for seed in range(20261, 20261 + 16):   # an image set on which an alpha sits on a grid boundary is replaced by the next seed's
        rng = np.random.default_rng(seed)
        try:
            out = _niqe_cases(nq, rng, mu, cov)
            break
        except ContestedAlpha as e:
            print(f"seed {seed}: {e}, trying the next")
    else:
        raise SystemExit("no uncontested image set among 16 seeds")
    out["seed"] = np.int64(seed)
    np.savez_compressed(os.path.join(GOLDEN, "niqe.npz"), **out)


def main():
    torch.set_num_threads(1)
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_import.REF
    nq, mf = load_reference(ref_root)
    gen_imresize(mf)
    gen_niqe(nq)
    for f in ("imresize.npz", "niqe.npz", "niqe_pris_params.npz"):
        print(f"wrote tests/golden/{f}: {os.path.getsize(os.path.join(GOLDEN, f))} bytes")


if __name__ == "__main__":
    main()
