"""GPU: the bf16 Restormer entry points stay inside their buffers.  The bf16 MDTA / GDFN forward and backward, the bf16 glue (convs,
pixel (un)shuffle, concat / split) and the edge convs run under the red zone (tests/redzone.py: exact-size workspaces and outputs with a
guard behind each, buffers pre-filled with NaN) at ragged shapes: the 32-pixel tiles of the per-head products against P = 63 / 260 / 129,
the per-row depthwise windows and the LayerNorm wave ranges at M not a multiple of 4; the wrapped tests also assert their accuracy, so a
read of memory no kernel wrote shows up as a NaN."""
import pytest
import torch

from redzone import redzone
from tests import test_gpu_restormer_bf16 as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def guarded(fn, *args):
    with redzone() as rz:
        fn(*args)
    assert rz.count > 0, "nothing was allocated through the patched helpers: the red zone checked nothing"


@pytest.mark.parametrize("lnt,dim,heads,B,H,W", [("BiasFree", 48, 1, 1, 13, 20), ("WithBias", 96, 2, 3, 7, 9), ("BiasFree", 192, 4, 1, 3, 43),
                                                  ("WithBias", 16, 2, 3, 5, 7)])
@pytest.mark.parametrize("variant", ["restormer", "promptir"])
def test_block_bf16(dev, lnt, dim, heads, B, H, W, variant):
    guarded(T.test_block_error_vs_fp64_within_naive_bf16_emulation, dev, lnt, dim, heads, B, H, W, variant)


@pytest.mark.parametrize("C,heads,B,H,W", [(48, 1, 3, 7, 9), (96, 2, 1, 13, 20)])
@pytest.mark.parametrize("save", ["full", "lean"])
def test_mdta_bf16_saved_modes(dev, C, heads, B, H, W, save):
    guarded(T.test_mdta_bf16_backward_vs_exact_on_own_forward, dev, C, heads, B, H, W, save, False)


def test_glue_bf16(dev):
    guarded(T.test_glue_bf16_vs_fp32, dev)


@pytest.mark.parametrize("name", ["Restormer", "Restormer_origin"])
@pytest.mark.parametrize("B,H,W", [(1, 24, 40), (3, 8, 56)])
def test_network_step_bf16(dev, name, B, H, W):
    """a whole training step of the tiny net (patch_embed, 8 blocks, Down/Upsample, concat, reduce_chan, output conv) at odd coarse grids
    (level 3: 3 x 5 / 1 x 7), balanced save mode"""
    def step():
        net = T._net(name, dev, act_dtype="bf16", save_mode="balanced")
        x = T.keyed_input("rzn.x", (B, 3, H, W)).to(dev)
        gw = T.keyed_input("rzn.gw", (B, 3, H, W), lo=-1.0, hi=1.0).to(dev)
        y, dx, grads = T._step(net, x, gw)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())

    guarded(step)
