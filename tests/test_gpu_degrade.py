"""GPU: the demosaic and line-mask degradations on the fused kernels of dcpt_amd/csrc/degrade.hip (through dcpt_amd.functional.demosaic /
inpaint_lines, basicsr.utils.dm / dm_matlab, the ``device`` backends of PairedImageMosaicDataset / PairedImageInpaintingDataset and the
models' ``feed_data``) against tests/degrade_restatement.py, the kernel-blind integer restatement on the CPU, and against the golden vectors
of the reference's mosaic_util (tests/golden/mosaic.npz).

Bounds:
* ``uint8_io`` and the line mask are integer-exact: compared BIT FOR BIT, nothing excluded.
* the float path: a Malvar output is a 13-term fp32 sum of dyadic weights, so it lies within 13 * 2^-24 * sum|w| * max|x| of the exact
  sum, sum|w| <= 2.5: 1.94e-6 * max|x|; bilinear has fewer terms.  Against the reference's own fp32 outputs, which carry the same error,
  twice that.

Every float case prints its figure before it asserts."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import degrade_restatement as R
from dcpt_amd.keyed_init import keyed_input
from tests.test_degrade_cpu import GOLDEN_CASES, golden_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_BOUND = 13 * 2.0 ** -24 * 2.5   # 1.94e-6, times max|x|
# (B, H, W): every tap reflected; the smallest even size; odd both ways; ragged in the tile; one more than the 16 x 64 tile each way, so
# halos cross tile edges and four tiles meet; three different images in one launch
SHAPES = {"3x3": (1, 3, 3), "4x4": (1, 4, 4), "5x7": (1, 5, 7), "17x33": (1, 17, 33), "tile+1": (1, 17, 65), "b3": (3, 10, 12)}
NAF_SMALL = ["network_g:width=8", "network_g:enc_blk_nums=[1,1,1,1]"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _input(name, channels):
    b, h, w = SHAPES[name]
    return keyed_input(f"gpudegrade.{name}.c{channels}", (b, channels, h, w), lo=-0.1, hi=1.1)   # (some samples beyond the clamp)


_REF = {}


def _reference(name, channels, method):
    """the restatement's uint8_io result for a case: computed once and shared"""
    key = (name, channels, method)
    if key not in _REF:
        _REF[key] = R.demosaic_u8(_input(name, channels).numpy(), method)
    return _REF[key]


@pytest.mark.parametrize("method", ["malvar", "bilinear"])
@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_demosaic_uint8_io_is_bit_identical_to_the_restatement(name, channels, method, dev):
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    x = _input(name, channels)
    want, sums, unit = _reference(name, channels, method)
    with kernel_trace() as t:
        y = DF.demosaic(x.to(dev), method, uint8_io=True).cpu()
    assert t.counts == {"degrade.demosaic": 1}, t.counts
    b, h, w = SHAPES[name]
    assert y.dtype == torch.float32 and tuple(y.shape) == (b, 3, h, w) and y.is_contiguous()
    wrong = int((_bits(y) != torch.from_numpy(want.view(np.int32))).sum())
    ties = int(((sums % unit) * 2 == unit).sum())
    print(f"demosaic uint8_io {name} C={channels} {method}: {wrong} of {y.numel()} elements differ; {ties} rounding ties in the case")
    assert wrong == 0


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_demosaic_float_path_against_the_reference_in_float64(tag, dev, golden_dir):
    """the 8-bit image of the golden case as fp32 values 0..255 (max|x| up to 255): RGB in (the mosaic fused) and the CFA plane in; integer
    inputs make every fp32 sum exact, so the keyed [0, 1] image is run as well"""
    from dcpt_amd import functional as DF

    x, g = golden_case(golden_dir, tag)
    u8 = torch.from_numpy(np.rint(x * 255).astype(np.float32))
    cfa = torch.from_numpy(g["cfa"].astype(np.float32))[:, None]
    peak = float(u8.max())
    for method in ("malvar", "bilinear"):
        want = torch.from_numpy(g[f"{method}64"])
        for name, inp in (("rgb", u8), ("cfa", cfa)):
            y = DF.demosaic(inp.to(dev), method).cpu()
            d = float((y.double() - want).abs().max())
            print(f"demosaic fp32 {tag} {method} {name}: max |d| {d:.3e} (bound {FLOAT_BOUND * peak:.3e} = 1.94e-6 x {peak:.0f})")
            assert d <= FLOAT_BOUND * peak
        assert float(want.min()) < 0 or float(want.max()) > 255 or method == "bilinear"   # no clamp on this path: overshoots survive
        # the keyed [0, 1] image itself (no 8-bit grid: the fp32 sums round) against the restatement's float64 sums
        y = DF.demosaic(torch.from_numpy(x).to(dev), method).cpu()
        d = float((y.double() - torch.from_numpy(R.demosaic_f64(x, method))).abs().max())
        print(f"demosaic fp32 {tag} {method} keyed [0, 1] input: max |d| {d:.3e} (bound {FLOAT_BOUND * float(np.abs(x).max()):.3e})")
        assert d <= FLOAT_BOUND * float(np.abs(x).max())


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_dm_wrappers_match_the_reference(tag, dev, golden_dir):
    from basicsr.utils import dm, dm_matlab

    x, g = golden_case(golden_dir, tag)

    def pack(plane):
        return torch.stack([plane[:, 0::2, 0::2], plane[:, 0::2, 1::2], plane[:, 1::2, 0::2], plane[:, 1::2, 1::2]], dim=1).to(dev)

    keyed = torch.from_numpy(R.cfa_of(x))
    for name, fn in (("malvar", dm_matlab), ("bilinear", dm)):
        y = fn(pack(torch.from_numpy(g["cfa"].astype(np.float32)))).cpu()
        d = float((y.double() - torch.from_numpy(g[f"{name}64"])).abs().max())
        y32 = fn(pack(keyed)).cpu()
        d32 = float((y32.double() - torch.from_numpy(g[f"{name}32"]).double()).abs().max())
        print(f"{fn.__name__} {tag}: against float64 on the 8-bit CFA {d:.3e} (bound {FLOAT_BOUND * 255:.3e}); against the reference's fp32 "
              f"on the keyed CFA {d32:.3e} (bound {2 * FLOAT_BOUND:.3e})")
        assert tuple(y.shape) == GOLDEN_CASES[tag] and d <= FLOAT_BOUND * 255 and d32 <= 2 * FLOAT_BOUND


# ---- the line mask ------------------------------------------------------------------------------------
def _strokes(h, w):
    """B = 4: n_lines 0, 5, 10, 10; thick 5, 10, 1, 7; both colours; a zero-length stroke; endpoints at (W, H) and (0, 0); a stroke in the
    far corner, off the first workgroup's 4 x 64 pixels wherever the plane has more than one"""
    rs = np.random.RandomState(h * 1000 + w)
    lines = np.stack([rs.randint(0, w + 1, (4, 10)), rs.randint(0, h + 1, (4, 10)), rs.randint(0, w + 1, (4, 10)),
                      rs.randint(0, h + 1, (4, 10))], axis=-1).astype(np.int32)
    lines[1, 0] = (w // 2, h // 2, w // 2, h // 2)
    lines[1, 1] = (w, h, 0, 0)
    lines[2, 0] = (w - 1, h - 1, w, h)
    lines[2, 1:] = lines[2, 0]                      # (thick 1, nothing else: the mask is the far corner alone)
    lines[3, 9] = (0, h, w, 0)
    meta = np.array([[0, 5, 1], [5, 10, 1], [10, 1, 0], [10, 7, 0]], dtype=np.int32)
    return torch.from_numpy(lines), torch.from_numpy(meta)


INPAINT_SHAPES = [(1, 1), (16, 16), (37, 65)]
_REF_INPAINT = {}


def _inpaint_case(h, w, channels):
    key = (h, w, channels)
    if key not in _REF_INPAINT:
        x = keyed_input(f"gpudegrade.inpaint.{h}x{w}.c{channels}", (4, channels, h, w), lo=-0.2, hi=1.2)
        lines, meta = _strokes(h, w)
        _REF_INPAINT[key] = (x, lines, meta, *R.inpaint(x.numpy(), lines.numpy(), meta.numpy()))
    return _REF_INPAINT[key]


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("shape", INPAINT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_inpaint_lines_is_bit_identical_to_the_restatement(shape, channels, dev):
    from kernel_trace import kernel_trace

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    h, w = shape
    x, lines, meta, want, masks = _inpaint_case(h, w, channels)
    want = torch.from_numpy(want.view(np.int32))
    xd = x.to(dev)
    with kernel_trace() as t:
        y = DF.inpaint_lines(xd, lines, meta)                      # host parameters: validated, copied
        y2 = DF.inpaint_lines(xd, lines.to(dev), meta.to(dev))     # device parameters
    assert t.counts == {"degrade.inpaint_lines": 2}, t.counts
    assert torch.equal(_bits(xd.cpu()), _bits(x)) and y.data_ptr() != xd.data_ptr()   # out of place: x untouched
    assert torch.equal(_bits(y.cpu()), want) and torch.equal(_bits(y2.cpu()), want)
    z = xd.clone()                                                 # in place: x == y at the entry point
    DF._call(_lib.load().dcpt_inpaint_lines_fwd, (z, lines.to(dev), meta.to(dev), z), (4, channels, h, w), dev)
    assert torch.equal(_bits(z.cpu()), want)
    share = [float(m.mean()) for m in masks]
    print(f"inpaint_lines {h}x{w} C={channels}: masked share per image {[round(s, 3) for s in share]}")
    assert share[0] == 0.0 and share[1] > 0 and share[3] > 0
    if (h, w) == (37, 65):
        assert masks[2].any() and not masks[2][:4, :64].any()      # the far-corner stroke lies wholly off the first workgroup's pixels


def test_inpaint_lines_validates_host_parameters(dev):
    from dcpt_amd import functional as DF

    x = keyed_input("gpudegrade.inpaint.bad", (1, 3, 8, 8)).to(dev)
    lines, meta = torch.zeros((1, 10, 4), dtype=torch.int32), torch.tensor([[5, 5, 1]], dtype=torch.int32)
    for bad_meta in ([[11, 5, 1]], [[-1, 5, 1]], [[5, 0, 1]], [[5, 65, 0]]):
        with pytest.raises(ValueError, match="n_lines|thick"):
            DF.inpaint_lines(x, lines, torch.tensor(bad_meta, dtype=torch.int32))
    far = lines.clone()
    far[0, 0, 2] = 16385
    with pytest.raises(ValueError, match="endpoint"):
        DF.inpaint_lines(x, far, meta)
    with pytest.raises(ValueError):
        DF.inpaint_lines(x, lines[:, :9], meta)
    with pytest.raises(ValueError):
        DF.inpaint_lines(x, lines.float(), meta)
    with pytest.raises(ValueError, match="method"):
        DF.demosaic(x, "ea")
    with pytest.raises(ValueError):
        DF.demosaic(x[:, :2])
    with pytest.raises(ValueError):
        DF.demosaic(x[:, :, :2])
    with pytest.raises(NotImplementedError, match="inference-only"):
        DF.demosaic(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="inference-only"):
        DF.inpaint_lines(x.clone().requires_grad_(True), lines, meta)
    # a device tensor is not read back: the kernel clamps n_lines 12 -> 10 and thick 100 -> 64, which covers an 8 x 8 plane
    y = DF.inpaint_lines(x, torch.full((1, 10, 4), 4, dtype=torch.int32, device=dev), torch.tensor([[12, 100, 1]], dtype=torch.int32, device=dev))
    assert bool((y == 1).all())


def test_outputs_stay_inside_their_buffers(dev):
    """both entry points on outputs of exactly the size they need, with a guard behind them, at ragged shapes; the outputs start as a NaN
    pattern, so a pixel a kernel skipped would show"""
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    x = _input("tile+1", 3).to(dev)
    b, h, w = SHAPES["tile+1"]
    xi, lines, meta, want, _ = _inpaint_case(37, 65, 3)
    xi, lines, meta = xi.to(dev), lines.to(dev), meta.to(dev)
    refs = {m: torch.from_numpy(_reference("tile+1", 3, m)[0].view(np.int32)).reshape(-1) for m in ("malvar", "bilinear")}
    with redzone() as rz:
        for flags, m in ((2, "malvar"), (3, "bilinear")):
            buf = DF._workspace(dev, 4 * b * 3 * h * w)
            DF._call(lib.dcpt_demosaic_fwd, (x, buf), (b, 3, h, w, flags), dev)
            assert torch.equal(buf.view(torch.int32).cpu(), refs[m])
        buf = DF._workspace(dev, 4 * xi.numel())
        DF._call(lib.dcpt_inpaint_lines_fwd, (xi, lines, meta, buf), (4, 3, 37, 65), dev)
        assert torch.equal(buf.view(torch.int32).cpu(), torch.from_numpy(want.view(np.int32)).reshape(-1))
    assert rz.count == 3


# ---- the data sets and the models' feed_data ----------------------------------------------------------------
@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("degrade_gt")
    for i, (h, w) in enumerate([(40, 48), (33, 37), (48, 35), (36, 36)]):
        low = keyed_input(f"gpudegrade.png{i}", (1, 3, h // 4 + 1, w // 4 + 1))
        img = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
        img = (img + keyed_input(f"gpudegrade.png{i}.n", (3, h, w), lo=-0.05, hi=0.05)).clamp(0, 1)
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(root / f"im{i}.png")
    return str(root)


def test_feed_data_on_a_device_batch_equals_the_host_backend(png_folder, dev):
    """the same sample through both backends: ``lq`` made by the kernel in SRModel.feed_data equals the worker's ``lq`` bit for bit"""
    from kernel_trace import kernel_trace

    from basicsr.data import build_dataloader, build_dataset
    from tests.test_gpu_jpeg import _sr_model

    model = _sr_model()
    cases = [("PairedImageMosaicDataset", "demosaic_backend", dict(demosaic_method="malvar"), "degrade.demosaic"),
             ("PairedImageMosaicDataset", "demosaic_backend", dict(demosaic_method="bilinear"), "degrade.demosaic"),
             ("PairedImageInpaintingDataset", "inpaint_backend", {}, "degrade.inpaint_lines")]
    for kind, key, extra, family in cases:
        sets = {b: build_dataset(dict(name=kind, type=kind, dataroot_gt=png_folder, phase="val", **{key: b}, **extra)) for b in ("host", "device")}
        for i in range(4):
            batches = {}
            for b, ds in sets.items():
                random.seed(31 + i)
                batches[b] = next(iter(build_dataloader(torch.utils.data.Subset(ds, [i]), dict(phase="val"))))
            assert "lq" not in batches["device"] and "lq" in batches["host"]
            with kernel_trace() as t:
                model.feed_data(batches["device"])
            assert t.counts == {family: 1}, t.counts
            assert torch.equal(_bits(model.lq.cpu()), _bits(batches["host"]["lq"])), (kind, extra, i)
            assert torch.equal(model.gt.cpu(), batches["host"]["gt"]) and not torch.equal(model.lq, model.gt)
    with pytest.raises(ValueError, match="one demosaic method"):
        model.feed_data({"gt": batches["host"]["gt"], "mosaic": torch.tensor([2], dtype=torch.int32)})


# ---- the command line on the shipped option files ------------------------------------------------------
def _cli(script, yml, over, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "basicsr", script), "-opt", yml, "--force_yml", *over], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-3000:]
    return out


def test_train_cli_on_the_demosaic_options(png_folder):
    """``python basicsr/train.py -opt options/demosaic/train_NAFNet_demosaic.yml`` shortened through --force_yml to two iterations on a
    temporary PNG folder: PairedImageMosaicDataset with ``demosaic_backend: device`` -> collate -> SRModel.feed_data -> the demosaic kernel;
    a second run reports the same numbers"""
    yml = os.path.join(ROOT, "options", "demosaic", "train_NAFNet_demosaic.yml")
    exp = os.path.join(ROOT, "experiments", "NAFNet_demosaic")
    over = [*NAF_SMALL, f"datasets:train:dataroot_gt={png_folder}", "datasets:train:gt_size=32", "datasets:train:batch_size_per_gpu=2",
            f"datasets:val_1:dataroot_gt={png_folder}", "train:total_iter=2", "train:scheduler:periods=[2]", "logger:print_freq=1",
            "logger:save_checkpoint_freq=2", "val:val_freq=2"]
    runs = []
    try:
        for _ in range(2):
            shutil.rmtree(exp, ignore_errors=True)
            out = _cli("train.py", yml, over)
            assert "Dataset [PairedImageMosaicDataset] - DFWB is built." in out and "Dataset [PairedImageMosaicDataset] - Kodak24 is built." in out
            losses = [float(v) for v in re.findall(r"l_pix: ([-0-9.eE+]+)", out)]
            assert len(losses) == 2 and all(0.0 < v < 2.0 for v in losses), out[-2000:]
            psnr = [float(v) for v in re.findall(r"#\s*psnr:\s*([-0-9.eE+]+)", out)]
            assert psnr and all(5.0 < v < 80.0 for v in psnr), out[-2000:]
            assert os.path.exists(os.path.join(exp, "models", "net_g_2.pth"))
            runs.append((losses, psnr))
        assert runs[0] == runs[1], runs
    finally:
        shutil.rmtree(exp, ignore_errors=True)


def test_test_cli_on_the_inpainting_options(png_folder):
    """``python basicsr/test.py -opt options/inpainting/test_NAFNet_inpainting.yml`` on the same folder: one set through the kernel, one
    through the host mask, the same strokes (``stroke_seed``): the same metrics from both, and from a second run"""
    yml = os.path.join(ROOT, "options", "inpainting", "test_NAFNet_inpainting.yml")
    over = [*NAF_SMALL, f"datasets:test_1:dataroot_gt={png_folder}", f"datasets:test_2:dataroot_gt={png_folder}"]
    res = os.path.join(ROOT, "results", "NAFNet_inpainting")
    runs = []
    try:
        for _ in range(2):
            out = _cli("test.py", yml, over)
            assert out.count("Dataset [PairedImageInpaintingDataset]") == 2
            vals = {}
            for chunk in out.split("Validation ")[1:]:
                for metric, v in re.findall(r"#\s*(psnr|ssim):\s*([-0-9.eE+]+)", chunk[:200]):
                    vals[(chunk.split()[0], metric)] = float(v)
            assert {("CBSD68", "psnr"), ("CBSD68", "ssim"), ("CBSD68_host", "psnr"), ("CBSD68_host", "ssim")} <= set(vals), out[-1500:]
            for (name, metric), v in vals.items():
                assert (0.0 < v <= 1.0) if metric == "ssim" else (5.0 < v < 80.0), (name, metric, v)
            assert vals[("CBSD68", "psnr")] == vals[("CBSD68_host", "psnr")] and vals[("CBSD68", "ssim")] == vals[("CBSD68_host", "ssim")]
            runs.append(vals)
        assert runs[0] == runs[1]
    finally:
        shutil.rmtree(res, ignore_errors=True)
