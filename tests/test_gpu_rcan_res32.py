"""GPU: RCAN inference on bf16 maps around an fp32 residual stream (``RCAN(act_dtype="bf16_res32")`` over dcpt_rcab_fwd_bf16_res32 and
dcpt_conv3x3_res_fwd_bf16_res32, the EB_RESID32 epilogue of the 128-row bf16 GEMM).

Yardstick and restatements: tests/res32_common.py -- err(HIP) <= 1.5 err(naive) + 4e-3 against the golden vector (or float64), where naive
rounds to bf16 at every storage point EXCEPT the stream.  Every case prints the three numbers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor
from res32_common import BF, cpu_sd, err, ident, naive_and_truth, rcan_net, rcan_rcab, rnd_bf16, yardstick

pytestmark = pytest.mark.gpu
TINY = dict(num_in_ch=3, num_out_ch=3, num_feat=32, num_group=2, num_block=2)
TINY_LR = (2, 3, 11, 13)
MODE = "bf16_res32"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _net(cfg, dev, seed=0, act_dtype=MODE):
    from basicsr.archs import build_network

    net = build_network(dict(type="RCAN", act_dtype=act_dtype, **cfg))
    fill_module_(net, seed=seed)
    return net.to(dev).eval()


def _rcab(C_, sq, rs, dev, tag=None, seed=0):
    from basicsr.archs.rcan_arch import RCAB

    blk = RCAB(C_, sq, rs)
    if tag is not None:
        blk.load_state_dict({k: keyed_tensor(f"rcab_{tag}." + k, tuple(v.shape)) for k, v in blk.state_dict().items()}, strict=True)
    else:
        fill_module_(blk, seed=seed)
    return blk.to(dev).eval()


def _stream(x, dev):
    """a CPU fp32 NCHW tensor as the fp32 channels_last stream and its bf16 image"""
    from dcpt_amd import functional as DF

    s = x.to(dev).contiguous(memory_format=torch.channels_last)
    return DF.Stream32(s, s.to(BF))


def _run_block(blk, x, dev):
    from kernel_trace import kernel_trace

    with torch.no_grad(), kernel_trace() as tr:
        y = blk(_stream(x, dev))
        torch.cuda.synchronize()
    assert y.s.dtype == torch.float32 and y.sb.dtype == BF and y.s.shape == x.shape == y.sb.shape
    assert tr["rcan_bf16.rcab_fwd_res32"] == 1 and tr["rcan_bf16.scale_res32"] == 1 and tr["nt_bf16.128_conv3"] == 2, tr.counts
    tr.assert_not_ran("rcan_bf16.rcab_fwd", "rcan_rcab_fwd", "nt_bf16.256_conv3", "nt_bf16.tall512_conv3")
    assert torch.equal(y.sb, y.s.to(BF)), "the bf16 image must be the rounded stream"
    return y.s


# ---- 1. RCAB at ragged shapes: M = 442 / 252 / 4495, none a multiple of 128 -------------------------------------------------------------------
@pytest.mark.parametrize("tag,C_,sq,B,H,W", [("c64_s16", 64, 16, 2, 13, 17), ("c32_s4", 32, 4, 2, 13, 17)])
def test_rcab_vs_golden(dev, golden_dir, tag, C_, sq, B, H, W):
    g = np.load(os.path.join(golden_dir, f"rcan_block_{tag}.npz"))
    blk = _rcab(C_, sq, 1.0, dev, tag=tag)
    x = keyed_input(f"rcab_{tag}.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    y = _run_block(blk, x, dev)
    naive, truth = naive_and_truth(lambda x_, P, rnd, srnd: rcan_rcab(x_, P, "", 1.0, rnd, srnd), x, cpu_sd(blk))
    assert err(truth, g["y"]) < 1e-5   # the float64 restatement is the reference's arithmetic
    yardstick(f"rcab {tag}", y, naive, g["y"])


@pytest.mark.parametrize("C_,sq,B,H,W", [(8, 8, 4, 7, 9), (64, 16, 5, 31, 29)])
def test_rcab_vs_float64(dev, C_, sq, B, H, W):
    blk = _rcab(C_, sq, 0.5, dev, seed=C_)
    x = keyed_input(f"rcanb{C_}", (B, C_, H, W), lo=-1.0, hi=1.0)
    y = _run_block(blk, x, dev)
    naive, truth = naive_and_truth(lambda x_, P, rnd, srnd: rcan_rcab(x_, P, "", 0.5, rnd, srnd), x, cpu_sd(blk))
    yardstick(f"rcab C={C_}", y, naive, truth)


# ---- 2. the residual conv, both output forms ----------------------------------------------------------------------------------------------------
def test_residual_conv_both_forms(dev):
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    C_, B, H, W = 64, 2, 13, 17
    w, b = keyed_tensor("resb.weight", (C_, C_, 3, 3)), keyed_tensor("resb.bias", (C_,))
    x = keyed_input("resb.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    res = keyed_input("resb.res", (B, C_, H, W), lo=-1.0, hi=1.0)
    with torch.no_grad():
        scale = float(F.conv2d(x, w, b, padding=1).abs().max())
    res = res * (8.0 * scale)   # a residual of another magnitude than the conv output
    xb = x.to(dev).to(BF).contiguous(memory_format=torch.channels_last)
    r32 = res.to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), kernel_trace() as tr:
        y, yb = DF.conv3x3_res_bf16_res32(xb, w.to(dev), b.to(dev), r32, out_f32=True, out_bf16=True)
        y_only, none_b = DF.conv3x3_res_bf16_res32(xb, w.to(dev), b.to(dev), r32)
        none_f, yb_only = DF.conv3x3_res_bf16_res32(xb, w.to(dev), b.to(dev), r32, out_f32=False, out_bf16=True)
        torch.cuda.synchronize()
    assert tr["rcan_bf16.res_fwd_res32"] == 3 and tr["nt_bf16.epi_resid32.128"] == 3 and tr["nt_bf16.128_conv3"] == 3, tr.counts
    tr.assert_not_ran("rcan_bf16.res_fwd", "nt_bf16.256_conv3")
    assert none_b is None and none_f is None and y.dtype == torch.float32 and yb.dtype == BF
    assert torch.equal(y_only, y) and torch.equal(yb_only, yb) and torch.equal(yb, y.to(BF))

    def conv(x_, P, rnd, srnd):
        return srnd(F.conv2d(rnd(x_), rnd(P["w"]), P["b"], padding=1) + P["res"])

    naive, truth = naive_and_truth(conv, x, {"w": w, "b": b, "res": res})
    yardstick("residual conv, fp32 out", y, naive, truth)
    yardstick("residual conv, bf16 out", yb_only, rnd_bf16(naive), truth)
    # the conv itself must be right too, not only the (larger) residual: the same bound on y - res at the conv output's scale
    yardstick("residual conv, conv part", y.cpu().double() - res.double(), naive.double() - res.double(), truth - res.double())


# ---- 3. the stream is not rounded ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,sq,B,H,W", [(64, 16, 2, 13, 17), (32, 4, 2, 13, 17)])
def test_rcab_with_zero_branch_returns_the_stream_exactly(dev, C_, sq, B, H, W):
    blk = _rcab(C_, sq, 0.5, dev, seed=3)
    with torch.no_grad():
        blk.rcab[2].weight.zero_()
        blk.rcab[2].bias.zero_()
    x = keyed_input(f"rcanexact{C_}", (B, C_, H, W), lo=-1.0, hi=1.0)
    assert not torch.equal(x.to(BF).float(), x), "the stream's values must not be bf16-representable"
    y = _run_block(blk, x, dev)
    assert torch.equal(y.cpu(), x), "S' must equal S bit for bit"


# ---- 4. nets --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_tiny_net_golden_trace_and_switching(dev, golden_dir, s):
    from kernel_trace import kernel_trace

    g = np.load(os.path.join(golden_dir, f"rcan_tiny_x{s}.npz"))
    cfg = dict(TINY, upscale=s)
    net = _net(cfg, dev)
    x = keyed_input(f"rcant{s}.x", TINY_LR)
    with torch.no_grad(), kernel_trace() as tr:
        y = net(x.to(dev))
        torch.cuda.synchronize()
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(g["y"].shape)
    nblk, ngrp = TINY["num_group"] * TINY["num_block"], TINY["num_group"]
    assert tr["rcan_bf16.rcab_fwd_res32"] == tr["rcan_bf16.scale_res32"] == nblk, tr.counts
    assert tr["rcan_bf16.res_fwd_res32"] == tr["nt_bf16.epi_resid32.128"] == ngrp + 1, tr.counts
    assert tr["rcan_bf16.ps_fwd"] == (2 if s == 4 else 1) and tr["edge.b2s_bf16"] == 1
    # no bf16-stream residual path and no fp32 RCAN kernel
    tr.assert_not_ran("rcan_bf16.rcab_fwd", "rcan_bf16.res_fwd", "rcan_rcab_fwd", "rcan_ps_fwd", "swin_conv3x3_res_fwd", "rcan_bf16.wpack_per_call",
                      "edge.s2b_bf16")
    naive, truth = naive_and_truth(rcan_net, x, cpu_sd(net), cfg, s)
    assert err(truth, g["y"]) < 1e-5
    yardstick(f"tiny x{s}", y, naive, g["y"])
    # the same object in the other two modes is bit-identical to a network never switched
    for act in ("bf16", "fp32"):
        net.set_act_dtype(act)
        fresh = _net(cfg, dev, act_dtype=act)
        with torch.no_grad(), kernel_trace() as tr:
            ya = net(x.to(dev))
            torch.cuda.synchronize()
        tr.assert_not_ran("rcan_bf16.rcab_fwd_res32", "rcan_bf16.res_fwd_res32", "nt_bf16.epi_resid32.128")
        with torch.no_grad():
            assert torch.equal(ya, fresh(x.to(dev))), act


def test_default_net_golden_and_purpose(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "rcan_full.npz"))
    cfg = dict(num_in_ch=3, num_out_ch=3)
    net = _net(cfg, dev)
    with torch.no_grad():   # tools/make_golden_rcan.py damp_, as tests/test_gpu_rcan.py::test_default_net_golden
        for k, p in net.named_parameters():
            if ".rcab.2." in k:
                p.mul_(0.1)
    assert list(net.state_dict().keys()) == list(g["keys"])
    x = keyed_input("rcanf.x", (1, 3, 12, 12))
    with torch.no_grad():
        y = net(x.to(dev))
        net.set_act_dtype("bf16")
        y16 = net(x.to(dev))
    naive, truth = naive_and_truth(rcan_net, x, cpu_sd(net), cfg, 4)
    assert err(truth[..., ::4, ::4], g["y_sub"]) < 1e-5
    e32 = yardstick("default net, bf16_res32", y[..., ::4, ::4], naive[..., ::4, ::4], g["y_sub"])
    e16 = err(y16[..., ::4, ::4], g["y_sub"])
    print(f"default net: err(HIP, bf16_res32) {e32:.3e}  err(HIP, bf16) {e16:.3e}")
    assert e32 < e16, "the fp32 stream must lower the error of the bf16 mode"


# ---- 5. determinism, batch consistency ----------------------------------------------------------------------------------------------------------
def test_determinism_and_batch_consistency(dev):
    net = _net(dict(TINY, upscale=3), dev)
    x = keyed_input("rcanbatch", (3, 3, 13, 10))
    with torch.no_grad():
        yb = net(x.to(dev))
        assert torch.equal(net(x.to(dev)), yb), "two runs must agree bit for bit"
        singles = torch.cat([net(x[i:i + 1].to(dev)) for i in range(3)], 0)
    assert bool(torch.isfinite(yb).all())
    assert torch.equal(yb, singles), "a batch of three must equal the three one-image forwards bit for bit"


# ---- 6. exact-size workspaces under red zones ----------------------------------------------------------------------------------------------------
def test_exact_workspaces_and_short_workspace_refused(dev):
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace
    from redzone import redzone

    lib = _lib.load()
    C_, sq, B, H, W = 64, 16, 2, 13, 17
    blk = _rcab(C_, sq, 1.0, dev, seed=7)
    st_ = _stream(keyed_input("rcanrz.x", (B, C_, H, W), lo=-1.0, hi=1.0), dev)
    c1 = blk.rcab[0]

    def run():
        y = blk(st_)
        a = DF.conv3x3_res_bf16_res32(st_.sb, c1.weight, c1.bias, st_.s, out_f32=True, out_bf16=True)
        b = DF.conv3x3_res_bf16_res32(st_.sb, c1.weight, c1.bias, st_.s, out_f32=False, out_bf16=True)
        return [y.s, y.sb, a[0], a[1], b[1]]

    with torch.no_grad():
        ref = run()
        with redzone() as rz:
            got = run()
        assert rz.count >= 8   # three workspaces, five outputs
    for a, b in zip(ref, got):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    # one byte short: refused before any launch
    ps = [t.detach() for t in (c1.weight, c1.bias, blk.rcab[2].weight, blk.rcab[2].bias, blk.rcab[3].attention[1].weight,
                               blk.rcab[3].attention[1].bias, blk.rcab[3].attention[3].weight, blk.rcab[3].attention[3].bias)]
    pp = _lib.RcabParams(*[t.data_ptr() for t in ps])
    y, yb = torch.empty_like(st_.s), torch.empty_like(st_.sb)
    st = torch.cuda.current_stream(dev).cuda_stream
    need = [lib.dcpt_rcab_bf16_res32_ws_bytes(B, H, W, C_, C_ // sq), lib.dcpt_conv3x3_res_bf16_res32_ws_bytes(B, H, W, C_)]
    assert min(need) > 0
    ws = torch.empty(max(need), dtype=torch.uint8, device=dev)
    with kernel_trace() as tr:
        rcs = [lib.dcpt_rcab_fwd_bf16_res32(C.byref(pp), None, 0, None, 0, st_.s.data_ptr(), st_.sb.data_ptr(), y.data_ptr(), yb.data_ptr(),
                                            ws.data_ptr(), need[0] - 1, B, H, W, C_, C_ // sq, 1.0, st),
               lib.dcpt_conv3x3_res_fwd_bf16_res32(st_.sb.data_ptr(), ps[0].data_ptr(), None, 0, ps[1].data_ptr(), st_.s.data_ptr(), y.data_ptr(),
                                                   yb.data_ptr(), ws.data_ptr(), need[1] - 1, B, H, W, C_, st)]
    assert all(rc != 0 for rc in rcs), rcs
    assert "workspace too small" in lib.dcpt_last_error().decode()
    assert tr.counts == {}, f"a refused call launched: {tr.counts}"


# ---- 7. SRModel ------------------------------------------------------------------------------------------------------------------------------------
def test_srmodel_tiled_inference_equals_tiles_alone(dev):
    """SRModel.test_tile with network_g.act_dtype: bf16_res32 at scale 4 (the sizes of the bf16 test): each tile's interior equals the network
    run on that padded tile alone, bit for bit"""
    from basicsr.models import build_model

    size, pad, s = 16, 4, 4
    opt = dict(name="t", model_type="SRModel", scale=4, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="RCAN", act_dtype=MODE, **dict(TINY, upscale=4)), path=dict(), val=dict(save_img=False),
               tile=dict(infer_size=size, tile_pad=pad))
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    assert m.net_g.act_dtype == MODE
    img = keyed_input("rcantile", (1, 3, 32, 48))
    m.feed_data({"lq": img})
    m.pre_test()
    m.test_tile()
    m.post_test()
    got = m.output.cpu()
    assert tuple(got.shape) == (1, 3, 128, 192)
    lq = img.to(dev)
    want = torch.zeros((1, 3, s * 32, s * 48))
    with torch.no_grad():
        for ty in range(2):
            for tx in range(3):
                x0, y0 = tx * size, ty * size
                xp0, yp0, xp1, yp1 = max(x0 - pad, 0), max(y0 - pad, 0), min(x0 + size + pad, 48), min(y0 + size + pad, 32)
                out = m.net_g(lq[:, :, yp0:yp1, xp0:xp1].contiguous())
                oy, ox = s * (y0 - yp0), s * (x0 - xp0)
                want[:, :, s * y0:s * (y0 + size), s * x0:s * (x0 + size)] = out[:, :, oy:oy + s * size, ox:ox + s * size].cpu()
    print(f"tiled vs tiles alone: {int((got != want).sum())} of {got.numel()} elements differ")
    assert torch.equal(got, want)
