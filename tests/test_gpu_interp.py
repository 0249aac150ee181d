"""GPU: the resize kernel of dcpt_amd/csrc/resize.hip (through dcpt_amd.functional.interpolate) against tests/interp_restatement.py, the
kernel-blind float64 numpy restatement of the header's arithmetic (tests/test_interp_cpu.py holds it against ``F.interpolate``).

Bound: kernel and restatement compute the same fp64 taps and the same sums up to the fusing of a multiply-add (relative 2^-53 per step,
about 1e-15 here), then round once to fp32: the results are equal or neighbouring fp32 values.  The inputs lie in [0, 1], so |v| < 2 also
with bicubic overshoot and a neighbour is at most 2^-23 away.

The kernel's output tile is T_H x T_W = 16 x 64.  1 x 9 -> 1 x 1 and 3 x 4: one lane, an area run longer than four taps, every clamp of
the bicubic taps; 5 x 7 by 1.5 and 0.5: one ragged tile; 67 x 131 by 0.15 (ratio 6.7, area runs of 7 and 8), by 0.37, by 1.23 (82 x 161:
6 x 3 tiles, the last of 2 rows and of 33 columns) and to 135 x 134 (9 x 3 tiles, the last of 7 rows and of 6 columns)."""
import numpy as np
import pytest
import torch

import interp_restatement as R
from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
T_H, T_W = 16, 64
BOUND = 2.0 ** -23
# name -> (shape, keywords)
CASES = {
    "1x9_to_1x1": ((1, 1, 1, 9), dict(size=(1, 1))),
    "1x9_to_3x4": ((1, 1, 1, 9), dict(size=(3, 4))),
    "5x7_by_1.5": ((2, 3, 5, 7), dict(scale_factor=1.5)),
    "5x7_by_0.5": ((2, 3, 5, 7), dict(scale_factor=0.5)),
    "67x131_by_0.15": ((2, 3, 67, 131), dict(scale_factor=0.15)),
    "67x131_by_0.37": ((2, 3, 67, 131), dict(scale_factor=0.37)),
    "67x131_by_1.23": ((2, 3, 67, 131), dict(scale_factor=1.23)),
    "67x131_to_135x134": ((2, 3, 67, 131), dict(size=(135, 134))),
    "67x131_to_24x48": ((2, 3, 67, 131), dict(size=(24, 48))),         # the output shape of 0.37 with the ratios of a size
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _input(name):
    shape = CASES[name][0]
    return keyed_input(f"gpuinterp.{shape}", shape)   # [0, 1]; one input per shape


_REF = {}


def reference(name, mode):
    """the restatement rounded to fp32 for a case: computed once, shared, never modified"""
    if (name, mode) not in _REF:
        _REF[name, mode] = torch.from_numpy(R.interp_f32(_input(name).numpy(), mode, **CASES[name][1]))
    return _REF[name, mode]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_restatement_and_repeats_bit_for_bit(name, mode, dev):
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    x = _input(name)
    xd = x.to(dev)
    with kernel_trace() as t:
        y = DF.interpolate(xd, mode=mode, **CASES[name][1])
        y2 = DF.interpolate(xd, mode=mode, **CASES[name][1])
    assert t.counts == {"degrade.interp": 2}, t.counts
    want = reference(name, mode)
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(want.shape) and y.is_contiguous()
    assert torch.equal(xd.cpu(), x)                       # x untouched
    d = float((y.cpu().double() - want.double()).abs().max())
    print(f"interpolate {name} {mode}: {tuple(x.shape)} -> {tuple(y.shape)}, max |d| {d:.3e} (bound {BOUND:.3e}), "
          f"{int((y.cpu() != want).sum())} of {want.numel()} differ")
    assert bool(torch.isfinite(y).all()) and d <= BOUND
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32))


@pytest.mark.parametrize("mode", R.MODES)
def test_a_scale_factor_and_a_size_of_one_shape_use_different_ratios(mode, dev):
    from dcpt_amd import functional as DF

    xd = _input("67x131_by_0.37").to(dev)
    by_scale, by_size = DF.interpolate(xd, scale_factor=0.37, mode=mode), DF.interpolate(xd, size=(24, 48), mode=mode)
    assert by_scale.shape == by_size.shape == (2, 3, 24, 48)
    for got, name in ((by_scale, "67x131_by_0.37"), (by_size, "67x131_to_24x48")):
        assert float((got.cpu().double() - reference(name, mode).double()).abs().max()) <= BOUND
    if mode == "area":                                    # adaptive pooling is made from the sizes alone
        assert torch.equal(by_scale, by_size)
    else:
        assert float((by_scale - by_size).abs().max()) > 1e-3


def test_exact_cases(dev):
    from dcpt_amd import functional as DF

    x = keyed_input("gpuinterp.exact", (2, 3, 37, 70), lo=-2.0, hi=2.0)
    xd = x.to(dev)
    for mode in R.MODES:
        assert torch.equal(DF.interpolate(xd, scale_factor=1.0, mode=mode).cpu(), x), mode
        assert torch.equal(DF.interpolate(xd, size=(37, 70), mode=mode).cpu(), x), mode
    k = torch.randint(0, 257, (2, 3, 34, 132), generator=torch.Generator().manual_seed(3)).float() / 256
    mean = (k[:, :, 0::2, 0::2] + k[:, :, 0::2, 1::2] + k[:, :, 1::2, 0::2] + k[:, :, 1::2, 1::2]) / 4   # exact in fp32
    assert torch.equal(DF.interpolate(k.to(dev), scale_factor=0.5, mode="area").cpu(), mean)
    assert torch.equal(DF.interpolate(k.to(dev), size=(17, 66), mode="area").cpu(), mean)
    wide = keyed_input("gpuinterp.grid", (2, 3, 37, 70), lo=-0.5, hi=1.5).to(dev)
    for mode in R.MODES:
        y = DF.interpolate(wide, scale_factor=1.23, mode=mode, clip=True, rounds=True)
        # the 8-bit grid as the header states it: float(k / 255.0) of an integer k, the division in fp64 (a device-side fp32 ``/ 255`` need
        # not be correctly rounded, so the grid is rebuilt on the host in float64)
        k = torch.round(y.cpu().double() * 255)
        assert float(y.min()) == 0.0 and float(y.max()) == 1.0 and float(k.min()) == 0 and float(k.max()) == 255, mode
        assert torch.equal(y.cpu(), (k / 255).float()), mode
        plain = DF.interpolate(wide, scale_factor=1.23, mode=mode)
        assert float((y - plain.clamp(0, 1)).abs().max()) <= 0.5 / 255 + 1e-6
        clipped = DF.interpolate(wide, scale_factor=1.23, mode=mode, clip=True)
        assert torch.equal(clipped, plain.clamp(0, 1))


def test_a_non_contiguous_input(dev):
    from dcpt_amd import functional as DF

    x = _input("67x131_by_0.37")
    t = x.to(dev).transpose(2, 3)                           # (2, 3, 131, 67), strided
    want = torch.from_numpy(R.interp_f32(x.transpose(2, 3).contiguous().numpy(), "bicubic", scale_factor=(0.5, 1.23)))
    got = DF.interpolate(t, scale_factor=(0.5, 1.23), mode="bicubic").cpu()
    assert got.shape == want.shape == (2, 3, 65, 82) and float((got.double() - want.double()).abs().max()) <= BOUND


def test_outputs_stay_inside_their_buffers(dev):
    """the entry point on outputs of exactly the size they need with a guard behind them, at ragged tiles; the outputs start as a NaN
    pattern, so an element the kernel skipped would show"""
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    with redzone() as rz:
        for name in ("1x9_to_3x4", "67x131_by_0.15", "67x131_by_1.23", "67x131_to_135x134"):
            x = _input(name)
            B, C, H, W = x.shape
            (Ho, Wo), (rh, rw) = DF.interp_geometry((H, W), **CASES[name][1])
            for m, mode in enumerate(DF.INTERP_MODES):
                buf = DF._workspace(dev, 4 * B * C * Ho * Wo)
                DF._call(lib.dcpt_interp_fwd, (x.to(dev), buf), (B, C, H, W, Ho, Wo, m, rh, rw, 0), dev)
                got = buf.view(torch.float32).reshape(B, C, Ho, Wo).cpu()
                assert float((got.double() - reference(name, mode).double()).abs().max()) <= BOUND, (name, mode)
    assert rz.count == 12


def test_refusals_of_the_python_op(dev):
    from dcpt_amd import functional as DF

    x = keyed_input("gpuinterp.bad", (2, 3, 8, 8)).to(dev)
    for kw, text in [(dict(), "exactly one"), (dict(size=4, scale_factor=0.5), "exactly one"), (dict(scale_factor=0.1), "must be positive"),
                     (dict(scale_factor=2.0, mode="nearest"), "mode must be"), (dict(size=(4, 4, 4)), "size must be")]:
        with pytest.raises(ValueError, match=text):
            DF.interpolate(x, **kw)
    with pytest.raises(ValueError, match="expected a non-empty"):
        DF.interpolate(x[0], scale_factor=2.0)
    with pytest.raises(NotImplementedError, match="inference-only"):
        DF.interpolate(x.clone().requires_grad_(True), scale_factor=2.0)
