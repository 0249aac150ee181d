"""GPU: SwinIR inference on bf16 maps around an fp32 residual stream (``SwinIR(act_dtype="bf16_res32")`` over dcpt_swin_attn_fwd_bf16_res32,
dcpt_swin_mlp_fwd_bf16_res32, dcpt_ln_pad_fwd_bf16_res32 and dcpt_conv3x3_res_fwd_bf16_res32 at the padded width).

Yardstick and restatements: tests/res32_common.py -- err(HIP) <= 1.5 err(naive) + 4e-3 against the golden vector (or float64), where naive
rounds to bf16 at every storage point EXCEPT the stream and knows nothing of padding.  Every case prints the three numbers.  Padded sizes are
read from the product (swinir_arch.pad8 / SwinIR.padded_dim)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor
from res32_common import BF, cpu_sd, err, naive_and_truth, swin_block_nchw, swin_net, yardstick

pytestmark = pytest.mark.gpu
MODE = "bf16_res32"
FULL = dict(embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
TINY = dict(embed_dim=36, depths=[2] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
FP32_SWIN_TAGS = ("swin_wattn_fwd", "swin_wattn_bwd", "swin_conv3x3_res_fwd", "swin_conv3x3_res_bwd")
BF16_STREAM_TAGS = ("swin_bf16.attn_fwd", "swin_bf16.mlp_fwd", "swin_bf16.ln_pad_fwd", "rcan_bf16.res_fwd")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _net(cfg, dev, act_dtype=MODE, seed=0):
    from basicsr.archs import build_network

    net = build_network(dict(type="SwinIR", act_dtype=act_dtype, **cfg))
    fill_module_(net, seed=seed)
    return net.to(dev).eval()


def _padded_stream(x, dev):
    """a CPU fp32 NCHW tensor as the zero-padded fp32 channels_last device stream"""
    from basicsr.archs.swinir_arch import pad8

    B, C_, H, W = x.shape
    xp = torch.zeros(B, pad8(C_), H, W)
    xp[:, :C_] = x
    return xp.to(dev).contiguous(memory_format=torch.channels_last)


def _pads_zero(y, C_):
    pad = y[:, C_:]
    return pad.numel() == 0 or bool((pad == 0).all())


def _block(C_, heads, ws, shift, dev, key):
    from basicsr.archs.swinir_arch import SwinTransformerBlock

    blk = SwinTransformerBlock(C_, (128, 128), heads, ws, shift, 2.0)
    blk.load_state_dict({k: keyed_tensor(key + k, tuple(v.shape)) for k, v in blk.state_dict().items()}, strict=True)
    return blk.to(dev).eval()


def _run_block(blk, x, dev):
    from basicsr.archs.swinir_arch import pad8
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    C_ = x.shape[1]
    with torch.no_grad(), kernel_trace() as tr:
        y = blk(DF.Stream32(_padded_stream(x, dev), None))
        torch.cuda.synchronize()
    assert y.s.dtype == torch.float32 and y.sb.dtype == BF and tuple(y.s.shape) == tuple(y.sb.shape) == (x.shape[0], pad8(C_), x.shape[2], x.shape[3])
    assert tr["swin_bf16.attn_fwd_res32"] == tr["swin_bf16.mlp_fwd_res32"] == tr["swin_bf16.wattn_fwd"] == 1, tr.counts
    assert tr["swin_bf16.ln_pad_fwd_f32in"] == 2 and tr["nt_bf16.epi_resid32.128"] == 2 and tr["nt_bf16.epi_biasgelu.128"] == 1, tr.counts
    assert tr["nt_bf16.128"] == 4 and tr["nt_bf16.256"] == 0 and tr["nt_bf16.tall512"] == 0, tr.counts
    tr.assert_not_ran(*FP32_SWIN_TAGS, *BF16_STREAM_TAGS)
    assert _pads_zero(y.s, C_), "pad columns of the stream must be exact zeros"
    assert torch.equal(y.sb, y.s.to(BF)), "the bf16 image must be the rounded stream"
    with torch.no_grad():   # the stream updated where it lies (what an RSTB does from its second block on): the same bits
        own = _padded_stream(x, dev)
        yi = blk._forward_res32(own, True, inplace=True)
    assert yi.s.data_ptr() == own.data_ptr() and torch.equal(yi.s, y.s) and torch.equal(yi.sb, y.sb), "in-place update differs"
    return y.s[:, :C_]


# ---- 1. blocks at ragged shapes -------------------------------------------------------------------------------------------------------------------
# c180 (Cp 184: the second column tile holds 56 of 128 columns; M = 192: one full and one ragged row tile), c60 / ws 4 with shifts 0 and ws / 2
GOLDEN_BLOCKS = [("c180_s0", 180, 6, 8, 0, 1, 8, 24), ("c180_s4", 180, 6, 8, 4, 1, 8, 24),
                 ("c60_ws4_s0", 60, 6, 4, 0, 2, 12, 16), ("c60_ws4_s2", 60, 6, 4, 2, 2, 12, 16)]


@pytest.mark.parametrize("tag,C_,heads,ws,shift,B,H,W", GOLDEN_BLOCKS)
def test_block_vs_golden(dev, golden_dir, tag, C_, heads, ws, shift, B, H, W):
    g = np.load(os.path.join(golden_dir, f"swinir_block_{tag}.npz"))
    blk = _block(C_, heads, ws, shift, dev, f"swb_{tag}.")
    x = keyed_input(f"swb_{tag}.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    y = _run_block(blk, x, dev)
    naive, truth = naive_and_truth(swin_block_nchw, x, cpu_sd(blk), heads, ws, shift)
    assert err(truth, g["y"]) < 1e-5   # the float64 restatement is the reference's arithmetic
    yardstick(f"block {tag}", y, naive, g["y"])


def test_block_c36_vs_float64(dev):
    C_, heads, ws, shift, B, H, W = 36, 6, 8, 0, 3, 8, 8   # Cp 40, hd 6 -> hdp 8, three images inside two row tiles
    blk = _block(C_, heads, ws, shift, dev, f"swb16_{C_}_{heads}.")
    x = keyed_input(f"swb16_{C_}_{heads}.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    y = _run_block(blk, x, dev)
    naive, truth = naive_and_truth(swin_block_nchw, x, cpu_sd(blk), heads, ws, shift)
    yardstick(f"block C={C_} heads={heads}", y, naive, truth)


# ---- 2. LayerNorm with fp32 input -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,Cp,M", [(180, 184, 97), (36, 40, 129), (64, 64, 128)])
def test_layernorm_fp32_rows(dev, C_, Cp, M):
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    x = keyed_input(f"swln{C_}.x", (M, Cp), lo=-2.0, hi=2.0)       # (the pad columns of the INPUT hold values: they must be ignored)
    assert not torch.equal(x.to(BF).float(), x)
    w, b = keyed_tensor(f"swln{C_}.w", (C_,)) + 1.0, keyed_tensor(f"swln{C_}.b", (C_,))
    wp, bp = torch.zeros(Cp), torch.zeros(Cp)
    wp[:C_], bp[:C_] = w, b
    xm = x.t().reshape(1, Cp, M, 1).to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), kernel_trace() as tr:
        y = DF.ln_pad_bf16_res32(xm, wp.to(dev), bp.to(dev), C_, 1e-5)
        torch.cuda.synchronize()
    assert tr["swin_bf16.ln_pad_fwd_f32in"] == 1 and tr["swin_bf16.ln_pad_fwd"] == 0 and tr["ln_fwd_bf16"] == 0
    assert y.dtype == BF
    y = y.reshape(Cp, M).t().cpu()
    assert bool((y[:, C_:].contiguous().view(torch.int16) == 0).all()) if Cp > C_ else True
    T = F.layer_norm(x[:, :C_].double(), (C_,), w.double(), b.double(), 1e-5)   # of the UNROUNDED rows
    d = (y[:, :C_].double() - T).abs()
    # one bf16 rounding of the result: half an ulp is at most 2^-8 |T|; 4e-6 of the scale for the fp32 arithmetic before it
    bound = 2.0 ** -8 * T.abs() + 4e-6 * float(T.abs().max())
    print(f"LayerNorm fp32 in {C_}/{Cp} M={M}: max |y - T| {float(d.max()):.3e}, worst ratio to its bound {float((d / bound).max()):.3f}")
    assert bool((d <= bound).all())


# ---- 3. the stream is not rounded -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,heads,ws,B,H,W", [(36, 6, 8, 3, 8, 8), (180, 6, 8, 1, 8, 24)])
def test_halves_with_zero_branch_return_the_stream_exactly(dev, C_, heads, ws, B, H, W):
    from basicsr.archs.swinir_arch import pad8
    from dcpt_amd import functional as DF

    blk = _block(C_, heads, ws, ws // 2, dev, f"swexact{C_}.")
    with torch.no_grad():
        for p in (blk.attn.proj.weight, blk.attn.proj.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias):
            p.zero_()
    blk.refresh_bf16()
    t = blk._swin_bf16.t
    x = keyed_input(f"swexact{C_}.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    assert not torch.equal(x.to(BF).float(), x), "the stream's values must not be bf16-representable"
    s = _padded_stream(x, dev)
    with torch.no_grad():
        ya = DF.swin_attn_bf16_res32(s, (t["norm1_w"], t["norm1_b"], t["qkv_w"], t["qkv_b"], t["proj_w"], t["proj_b"]), C_, heads, pad8(C_ // heads),
                                     ws, ws // 2)
        ym, ymb = DF.swin_mlp_bf16_res32(s, (t["norm2_w"], t["norm2_b"], t["fc1_w"], t["fc1_b"], t["fc2_w"], t["fc2_b"]), C_, out_bf16=True)
        ym2, none = DF.swin_mlp_bf16_res32(s, (t["norm2_w"], t["norm2_b"], t["fc1_w"], t["fc1_b"], t["fc2_w"], t["fc2_b"]), C_)
    assert none is None
    assert torch.equal(ya, s), "attention half with proj = 0: S' must equal S bit for bit"
    assert torch.equal(ym, s) and torch.equal(ym2, s), "MLP half with fc2 = 0: S' must equal S bit for bit"
    assert torch.equal(ymb, s.to(BF))
    assert pad8(C_) > C_ and _pads_zero(ya, C_) and _pads_zero(ym, C_)


# ---- 4. nets -----------------------------------------------------------------------------------------------------------------------------------------
def test_tiny_net_golden_trace_and_switching(dev, golden_dir):
    from kernel_trace import kernel_trace

    g = np.load(os.path.join(golden_dir, "swinir_tiny.npz"))
    net = _net(TINY, dev)
    x = keyed_input("swt.x", (2, 3, 32, 40))
    with torch.no_grad(), kernel_trace() as tr:
        y = net(x.to(dev))
        torch.cuda.synchronize()
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(g["y"].shape)
    nblk = sum(TINY["depths"])
    assert tr["swin_bf16.attn_fwd_res32"] == tr["swin_bf16.mlp_fwd_res32"] == tr["swin_bf16.wattn_fwd"] == nblk == 12, tr.counts
    assert tr["swin_bf16.ln_pad_fwd_f32in"] == 2 * nblk + 2 and tr["rcan_bf16.res_fwd_res32"] == 7, tr.counts
    assert tr["nt_bf16.epi_resid32.128"] == 2 * nblk + 7, tr.counts
    # no bf16-stream residual path and no fp32 Swin kernel
    tr.assert_not_ran("rcan_bf16.wpack_per_call", "edge.s2b_bf16", *FP32_SWIN_TAGS, *BF16_STREAM_TAGS)
    assert tr["edge.b2s_bf16"] == 1   # conv_last on the bf16-input edge kernel
    naive, truth = naive_and_truth(swin_net, x, cpu_sd(net), TINY)
    assert err(truth, g["y"]) < 1e-5
    yardstick("tiny net", y, naive, g["y"])
    # the same object in the other two modes is bit-identical to a network never switched
    for act in ("bf16", "fp32"):
        net.set_act_dtype(act)
        fresh = _net(TINY, dev, act_dtype=act)
        with torch.no_grad(), kernel_trace() as tr:
            ya = net(x.to(dev))
            torch.cuda.synchronize()
        tr.assert_not_ran("swin_bf16.attn_fwd_res32", "swin_bf16.ln_pad_fwd_f32in", "rcan_bf16.res_fwd_res32", "nt_bf16.epi_resid32.128")
        with torch.no_grad():
            assert torch.equal(ya, fresh(x.to(dev))), act


def test_default_net_golden_and_purpose(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "swinir_full.npz"))
    net = _net(FULL, dev)
    assert list(net.state_dict().keys()) == list(g["keys"]) and net.padded_dim() == 184
    x = keyed_input("swf.x", (1, 3, 64, 64))
    with torch.no_grad():
        y = net(x.to(dev))
        net.set_act_dtype("bf16")
        y16 = net(x.to(dev))
    naive, truth = naive_and_truth(swin_net, x, cpu_sd(net), FULL)
    assert err(truth[..., ::4, ::4], g["y_sub"]) < 1e-5
    e32 = yardstick("default net y_sub, bf16_res32", y[..., ::4, ::4], naive[..., ::4, ::4], g["y_sub"])
    e16 = err(y16[..., ::4, ::4], g["y_sub"])
    print(f"default net: err(HIP, bf16_res32) {e32:.3e}  err(HIP, bf16) {e16:.3e}")
    assert e32 < e16, "the fp32 stream must lower the error of the bf16 mode"


# ---- 5. determinism, batch consistency ------------------------------------------------------------------------------------------------------------
def test_determinism_and_batch_consistency(dev):
    net = _net(TINY, dev)
    x = keyed_input("swb16.batch", (3, 3, 24, 16))   # M = 384 per image: an image boundary inside a 128-row tile of the batch
    with torch.no_grad():
        yb = net(x.to(dev))
        assert torch.equal(net(x.to(dev)), yb), "two runs must agree bit for bit"
        singles = torch.cat([net(x[i:i + 1].to(dev)) for i in range(3)], 0)
    assert bool(torch.isfinite(yb).all())
    assert torch.equal(yb, singles), "a batch of three must equal the three one-image forwards bit for bit"


# ---- 6. exact-size workspaces under red zones -----------------------------------------------------------------------------------------------------
def test_exact_workspaces_and_short_workspace_refused(dev):
    from basicsr.archs.swinir_arch import pad8
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace
    from redzone import redzone

    lib = _lib.load()
    C_, heads, ws, shift, B, H, W = 180, 6, 8, 4, 1, 8, 24
    Cp, hdp, hidden = pad8(C_), pad8(C_ // heads), 2 * C_
    blk = _block(C_, heads, ws, shift, dev, "swrz.")
    x = _padded_stream(keyed_input("swrz.x", (B, C_, H, W), lo=-1.0, hi=1.0), dev)
    blk.refresh_bf16()
    t = blk._swin_bf16.t

    def run():
        y = blk(DF.Stream32(x, None))
        return [y.s, y.sb, DF.ln_pad_bf16_res32(x, t["norm1_w"], t["norm1_b"], C_)]

    with torch.no_grad():
        ref = run()
        with redzone() as rz:
            got = run()
        assert rz.count >= 5   # two workspaces, three outputs (the MLP half updates the attention half's output in place)
    for a, b in zip(ref, got):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    # one byte short: refused before any launch
    pa = _lib.SwinAttnBf16Params(*[t[k].data_ptr() for k in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b")])
    pm = _lib.SwinMlpBf16Params(*[t[k].data_ptr() for k in ("norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")])
    y = torch.empty_like(x)
    st = torch.cuda.current_stream(dev).cuda_stream
    need = [lib.dcpt_swin_attn_bf16_res32_ws_bytes(B, H, W, C_, Cp, heads, hdp, ws), lib.dcpt_swin_mlp_bf16_res32_ws_bytes(B, H, W, C_, Cp, hidden)]
    assert min(need) > 0
    wsb = torch.empty(max(need), dtype=torch.uint8, device=dev)
    with kernel_trace() as tr:
        rcs = [lib.dcpt_swin_attn_fwd_bf16_res32(C.byref(pa), x.data_ptr(), y.data_ptr(), wsb.data_ptr(), need[0] - 1, B, H, W, C_, Cp, heads, hdp,
                                                 ws, shift, st),
               lib.dcpt_swin_mlp_fwd_bf16_res32(C.byref(pm), x.data_ptr(), y.data_ptr(), None, wsb.data_ptr(), need[1] - 1, B, H, W, C_, Cp, hidden,
                                                st)]
    assert all(rc != 0 for rc in rcs), rcs
    assert "workspace too small" in lib.dcpt_last_error().decode()
    assert tr.counts == {}, f"a refused call launched: {tr.counts}"


# ---- 7. SRModel -----------------------------------------------------------------------------------------------------------------------------------
def test_srmodel_tiled_inference_equals_tiles_alone(dev):
    """SRModel.test_tile with network_g.act_dtype: bf16_res32 (the sizes of the bf16 test): each tile's interior equals the network run on that
    padded tile alone, bit for bit"""
    from basicsr.models import build_model

    size, pad = 8, 8
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="SwinIR", act_dtype=MODE, **TINY), path=dict(pretrain_network_g=None), val=dict(save_img=False),
               tile=dict(infer_size=size, tile_pad=pad))
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    assert m.net_g.act_dtype == MODE
    img = keyed_input("swtile16", (1, 3, 24, 24))
    m.feed_data({"lq": img})
    m.pre_test()
    m.test_tile()
    m.post_test()
    got = m.output.cpu()
    lq = img.to(dev)
    want = torch.zeros_like(img)
    with torch.no_grad():
        for ty in range(3):
            for tx in range(3):
                x0, y0 = tx * size, ty * size
                xp0, yp0, xp1, yp1 = max(x0 - pad, 0), max(y0 - pad, 0), min(x0 + size + pad, 24), min(y0 + size + pad, 24)
                out = m.net_g(lq[:, :, yp0:yp1, xp0:xp1].contiguous())
                want[:, :, y0:y0 + size, x0:x0 + size] = out[:, :, y0 - yp0:y0 - yp0 + size, x0 - xp0:x0 - xp0 + size].cpu()
    print(f"tiled vs tiles alone: {int((got != want).sum())} of {got.numel()} elements differ")
    assert torch.equal(got, want)
