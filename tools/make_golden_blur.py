"""Golden vectors of the reference's blur toolbox (build container only; needs the reference tree and scipy).

    python tools/make_golden_blur.py [REFERENCE_ROOT]

Loads the reference's basicsr/data/degradations.py and basicsr/utils/img_process_util.py by file path under private module names, with
``cv2`` and ``torchvision`` as empty stubs (the blur-kernel code and ``filter2D`` call neither).  Writes

  tests/golden/blur_kernels.npz   for each of the six ``random_mixed_kernels`` kinds at K = 7 and 21, and for ``random_bivariate_Gaussian`` /
                                  ``random_bivariate_generalized_Gaussian`` with ``noise_range=(0.75, 1.25)``: the seed, the arguments and
                                  the reference's float64 kernel; three ``circular_lowpass_kernel`` cases, one with ``pad_to``
  tests/golden/filter2d.npz       input, kernels and the reference's fp32 ``filter2D`` output on the CPU for (B, C, H, W, K) =
                                  (2, 3, 11, 13, 21) with per-image kernels, (2, 3, 9, 8, 5) with a shared kernel and (1, 1, 4, 5, 7);
                                  input and output of the reference's ``USMSharp.forward`` on a (2, 3, 24, 20) batch, called on an
                                  instance whose ``kernel`` buffer is this project's Gaussian at radius 11 (cv2 is never reached)

and prints what the tests' bounds are made of: per kernel case the largest deviation of this project's generator from the reference's
kernel, per ``filter2D`` case and for the USM case the largest deviation of the float64 restatement (tests/blur_restatement.py) from the
reference's fp32 output.  The USM mask is a step at ``|residual| * 255 = threshold``: the tool asserts that no pixel of the fixture lies
within 1e-3 of it (the seed is advanced until that holds with no pixel left out).  Single-threaded CPU, seeded: a rerun reproduces the
files."""
from __future__ import annotations

import importlib.util
import math
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import blur_restatement as R  # noqa: E402
from basicsr.data import degradations as G  # noqa: E402
from basicsr.utils.img_process_util import _gaussian_kernel2d  # noqa: E402
from oracle import ref_import  # noqa: E402  (REF: where the reference tree lives)

GOLDEN = os.path.join(ROOT, "tests", "golden")
KINDS = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")
MIXED_ARGS = dict(sigma_x_range=(0.6, 5.0), sigma_y_range=(0.4, 4.0), rotation_range=(-math.pi, math.pi), betag_range=(0.5, 4.0),
                  betap_range=(0.7, 2.0))
NOISE_RANGE = (0.75, 1.25)
SINC_CASES = [(math.pi / 3, 7, 0), (2.0, 21, 0), (0.9 * math.pi, 13, 21)]   # (cutoff, kernel_size, pad_to)
FILTER_CASES = [("per_image", (2, 3, 11, 13), 21, True), ("shared", (2, 3, 9, 8), 5, False), ("tiny", (1, 1, 4, 5), 7, True)]
USM_SHAPE, USM_RADIUS, USM_WEIGHT, USM_THRESHOLD = (2, 3, 24, 20), 11, 0.5, 10


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref_root):
    """-> (the reference's degradations module, its img_process_util module), loaded without its package __init__"""
    names = ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional")
    saved = {k: sys.modules[k] for k in list(sys.modules) if k == "cv2" or k == "torchvision" or k.startswith("torchvision.")}
    for k in saved:
        del sys.modules[k]
    try:
        for name in names:
            sys.modules[name] = types.ModuleType(name)
        sys.modules["torchvision.transforms.functional"].rgb_to_grayscale = None
        deg = _load("_ref_degradations", os.path.join(ref_root, "basicsr", "data", "degradations.py"))
        ipu = _load("_ref_img_process_util", os.path.join(ref_root, "basicsr", "utils", "img_process_util.py"))
        return deg, ipu
    finally:
        for k in [k for k in sys.modules if k == "cv2" or k == "torchvision" or k.startswith("torchvision.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def gen_kernels(deg):
    out, worst, seed = {}, 0.0, 4100
    for K in (7, 21):
        for kind in KINDS:
            seed += 1
            _seed(seed)
            ref = deg.random_mixed_kernels([kind], [1.0], K, noise_range=None, **MIXED_ARGS)
            _seed(seed)
            mine = G.random_mixed_kernels([kind], [1.0], K, noise_range=None, **MIXED_ARGS)
            dev = float(np.abs(mine - ref).max())
            worst = max(worst, dev)
            print(f"random_mixed_kernels {kind} K={K} seed {seed}: this project's generator against the reference {dev:.3e}, sum {ref.sum():.17g}")
            out[f"mixed.{kind}.{K}.kernel"], out[f"mixed.{kind}.{K}.seed"] = ref, np.int64(seed)
    for k, v in MIXED_ARGS.items():
        out[f"mixed.{k}"] = np.array(v, dtype=np.float64)
    for tag, K, iso in (("gauss_noise", 21, False), ("gauss_noise_iso", 7, True)):
        seed += 1
        a = (K, MIXED_ARGS["sigma_x_range"], MIXED_ARGS["sigma_y_range"], MIXED_ARGS["rotation_range"])
        _seed(seed)
        ref = deg.random_bivariate_Gaussian(*a, noise_range=NOISE_RANGE, isotropic=iso)
        _seed(seed)
        mine = G.random_bivariate_Gaussian(*a, noise_range=NOISE_RANGE, isotropic=iso)
        dev = float(np.abs(mine - ref).max())
        worst = max(worst, dev)
        print(f"random_bivariate_Gaussian noise K={K} isotropic={iso} seed {seed}: {dev:.3e}")
        out[f"{tag}.kernel"], out[f"{tag}.seed"], out[f"{tag}.K"], out[f"{tag}.isotropic"] = ref, np.int64(seed), np.int64(K), np.bool_(iso)
    for tag, K, iso in (("ggauss_noise", 21, False), ("ggauss_noise_iso", 7, True)):
        seed += 1
        a = (K, MIXED_ARGS["sigma_x_range"], MIXED_ARGS["sigma_y_range"], MIXED_ARGS["rotation_range"], MIXED_ARGS["betag_range"])
        _seed(seed)
        ref = deg.random_bivariate_generalized_Gaussian(*a, noise_range=NOISE_RANGE, isotropic=iso)
        _seed(seed)
        mine = G.random_bivariate_generalized_Gaussian(*a, noise_range=NOISE_RANGE, isotropic=iso)
        dev = float(np.abs(mine - ref).max())
        worst = max(worst, dev)
        print(f"random_bivariate_generalized_Gaussian noise K={K} isotropic={iso} seed {seed}: {dev:.3e}")
        out[f"{tag}.kernel"], out[f"{tag}.seed"], out[f"{tag}.K"], out[f"{tag}.isotropic"] = ref, np.int64(seed), np.int64(K), np.bool_(iso)
    out["noise_range"] = np.array(NOISE_RANGE, dtype=np.float64)
    for i, (cutoff, K, pad_to) in enumerate(SINC_CASES):
        ref = deg.circular_lowpass_kernel(cutoff, K, pad_to)
        dev = float(np.abs(G.circular_lowpass_kernel(cutoff, K, pad_to) - ref).max())
        worst = max(worst, dev)
        print(f"circular_lowpass_kernel cutoff={cutoff:.6f} K={K} pad_to={pad_to}: {dev:.3e}, shape {ref.shape}")
        out[f"sinc.{i}.kernel"], out[f"sinc.{i}.args"] = ref, np.array([cutoff, K, pad_to], dtype=np.float64)
    print(f"blur kernels: largest deviation {worst:.3e} (the tests' bound is 1e-12)")
    out["max_dev"] = np.float64(worst)
    np.savez_compressed(os.path.join(GOLDEN, "blur_kernels.npz"), **out)


def _image(rng, shape):
    """a batch in [0, 1] with image-like statistics: a smooth field plus fine texture"""
    B, C, H, W = shape
    low = torch.from_numpy(rng.random((B, C, H // 4 + 2, W // 4 + 2)))
    smooth = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).numpy()
    return np.clip(smooth + rng.normal(0, 0.04, shape), 0, 1).astype(np.float32)


def gen_filter2d(deg, ipu):
    out = {}
    rng = np.random.default_rng(5200)
    for i, (tag, shape, K, per_image) in enumerate(FILTER_CASES):
        x = rng.random(shape, dtype=np.float32)
        kern = []
        for b in range(shape[0] if per_image else 1):   # anisotropic kernels of the reference: non-negative, sum 1, no symmetry under a flip
            _seed(5300 + 10 * i + b)
            kern.append(deg.random_mixed_kernels(["aniso", "generalized_aniso"], [0.5, 0.5], K, noise_range=NOISE_RANGE, **MIXED_ARGS))
        kern = np.stack(kern).astype(np.float32)
        y = ipu.filter2D(torch.from_numpy(x), torch.from_numpy(kern)).numpy()
        dev = float(np.abs(R.filter2d(x, kern) - y).max())
        print(f"filter2D {tag} {shape} K={K}: float64 restatement against the reference's fp32 output {dev:.3e} (bound K^2 2^-24 = {K * K * 2.0 ** -24:.3e})")
        out[f"{tag}.x"], out[f"{tag}.kernel"], out[f"{tag}.y"] = x, kern, y
    kernel = torch.from_numpy(_gaussian_kernel2d(USM_RADIUS, 0)).unsqueeze(0)
    usm = ipu.USMSharp.__new__(ipu.USMSharp)   # (its __init__ calls cv2.getGaussianKernel)
    torch.nn.Module.__init__(usm)
    usm.radius = USM_RADIUS
    usm.register_buffer("kernel", kernel)
    for seed in range(5400, 5400 + 64):
        img = _image(np.random.default_rng(seed), USM_SHAPE)
        blur = R.filter2d(img, kernel.numpy())
        margin = np.abs(np.abs(img.astype(np.float64) - blur) * 255 - USM_THRESHOLD)
        if float(margin.min()) >= 1e-3:
            break
        print(f"usm seed {seed}: a pixel {float(margin.min()):.2e} from the mask's step, trying the next")
    else:
        raise SystemExit("no USM image among 64 seeds keeps every pixel off the mask's step")
    assert not (margin < 1e-3).any()
    y = usm(torch.from_numpy(img), weight=USM_WEIGHT, threshold=USM_THRESHOLD).numpy()
    mine = R.usm_sharp(torch.from_numpy(img), kernel, USM_WEIGHT, USM_THRESHOLD).numpy()
    on = float((np.abs(img.astype(np.float64) - blur) * 255 > USM_THRESHOLD).mean())
    print(f"USMSharp radius {USM_RADIUS} seed {seed}: closest pixel to the step {float(margin.min()):.3e}, {100 * on:.1f} % of the mask set; "
          f"restatement against the reference's output {float(np.abs(mine.astype(np.float64) - y).max()):.3e} "
          f"(bound per blur K^2 2^-24 = {USM_RADIUS ** 2 * 2.0 ** -24:.3e})")
    out["usm.x"], out["usm.y"], out["usm.kernel"] = img, y, kernel.numpy()
    out["usm.args"] = np.array([USM_RADIUS, USM_WEIGHT, USM_THRESHOLD], dtype=np.float64)
    out["usm.seed"] = np.int64(seed)
    np.savez_compressed(os.path.join(GOLDEN, "filter2d.npz"), **out)


def main():
    torch.set_num_threads(1)
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_import.REF
    deg, ipu = load_reference(ref_root)
    gen_kernels(deg)
    gen_filter2d(deg, ipu)
    for f in ("blur_kernels.npz", "filter2d.npz"):
        print(f"wrote tests/golden/{f}: {os.path.getsize(os.path.join(GOLDEN, f))} bytes")


if __name__ == "__main__":
    main()
