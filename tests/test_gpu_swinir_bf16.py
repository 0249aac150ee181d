"""GPU: SwinIR inference on bf16 activation storage (``SwinIR(act_dtype="bf16")`` over dcpt_swin_attn_fwd_bf16, dcpt_swin_mlp_fwd_bf16,
dcpt_ln_pad_fwd_bf16 and the existing bf16 conv entry points at the padded width).

Accuracy yardstick (the project's own for bf16 storage, tests/test_gpu_bf16.py, tests/test_gpu_rcan_bf16.py): for a tensor with truth T,
    err(HIP) <= 1.5 * err(naive) + 4e-3,      err = max|. - T| / max|T|
4e-3 is one bf16 ulp at the tensor's scale, 1.5 covers the spread of a max-norm.  T is the golden vector of the real reference where
tests/golden holds one, else a float64 restatement without rounding.  ``naive`` is a kernel-blind fp32 torch restatement on the CPU, rounded to
torch.bfloat16 at exactly the documented storage points -- block input, weight operand images, LN output, qkv, P, attention output, proj +
residual, fc1 + GELU, fc2 + residual, conv outputs -- with fp32 biases, statistics, scores, softmax and accumulation.  It knows nothing of
padding: it works on the C real channels.  Every case prints the three numbers.

Padded sizes are read from the product (swinir_arch.pad8 / SwinIR.padded_dim), not assumed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FULL = dict(embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
TINY = dict(embed_dim=36, depths=[2] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
MEAN = (0.4488, 0.4371, 0.4040)
FP32_SWIN_TAGS = ("swin_wattn_fwd", "swin_wattn_bwd", "swin_conv3x3_res_fwd", "swin_conv3x3_res_bwd")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _np(a):
    return a.detach().float().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def err(a, T):
    a, T = _np(a), _np(T)
    assert a.shape == T.shape, (a.shape, T.shape)
    return float(np.abs(a - T).max() / max(1e-12, np.abs(T).max()))


def yardstick(name, hip, naive, T):
    eh, en = err(hip, T), err(naive, T)
    print(f"{name}: err(HIP) {eh:.3e}  err(naive) {en:.3e}  bound {1.5 * en + 4e-3:.3e}")
    assert np.isfinite(eh) and eh <= 1.5 * en + 4e-3, f"{name}: err(HIP) {eh:.3e} > 1.5 * err(naive) {en:.3e} + 4e-3"


# ---- the restatement: rnd = bf16 rounding at the storage points in fp32 (naive), or the identity in float64 (truth); CPU, unpadded --------------
def rnd_bf16(t):
    return t.to(BF).to(t.dtype)


def ident(t):
    return t


def re_block(x, P, pre, heads, ws, shift, rnd):
    """x (B, H, W, C): the block input as stored (already rnd'ed)"""
    B, H, W, C_ = x.shape
    hd = C_ // heads
    h = rnd(F.layer_norm(x, (C_,), P[pre + "norm1.weight"], P[pre + "norm1.bias"], 1e-5))
    if shift:
        h = torch.roll(h, (-shift, -shift), (1, 2))
    win = h.reshape(B, H // ws, ws, W // ws, ws, C_).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C_)
    qkv = rnd(F.linear(win, rnd(P[pre + "attn.qkv.weight"]), P[pre + "attn.qkv.bias"]))
    qkv = qkv.reshape(win.shape[0], ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
    p = rnd(torch.softmax((qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5, -1))
    o = rnd(p @ qkv[2]).transpose(1, 2).reshape(-1, ws * ws, C_)
    o = F.linear(o, rnd(P[pre + "attn.proj.weight"]), P[pre + "attn.proj.bias"])
    o = o.reshape(B, H // ws, W // ws, ws, ws, C_).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C_)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    t = rnd(x + o)
    m = rnd(F.layer_norm(t, (C_,), P[pre + "norm2.weight"], P[pre + "norm2.bias"], 1e-5))
    g = rnd(F.gelu(F.linear(m, rnd(P[pre + "mlp.fc1.weight"]), P[pre + "mlp.fc1.bias"])))
    return rnd(t + F.linear(g, rnd(P[pre + "mlp.fc2.weight"]), P[pre + "mlp.fc2.bias"]))


def re_block_nchw(x, P, heads, ws, shift, rnd):
    return re_block(rnd(x.permute(0, 2, 3, 1)), P, "", heads, ws, shift, rnd).permute(0, 3, 1, 2)


def re_net(x, P, cfg, rnd):
    ws = cfg["window_size"]
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    xn = x - mean

    def conv(t, pre, r=rnd):   # NHWC in / out; r: the rounding of the weight operand image (the edge convs read fp32 weights)
        return F.conv2d(t.permute(0, 3, 1, 2), r(P[pre + ".weight"]), P[pre + ".bias"], padding=1).permute(0, 2, 3, 1)

    def ln(t, pre):
        return rnd(F.layer_norm(t, (t.shape[-1],), P[pre + ".weight"], P[pre + ".bias"], 1e-5))

    xf = rnd(conv(xn.permute(0, 2, 3, 1), "conv_first", ident))
    t = ln(xf, "patch_embed.norm")
    n = len(cfg["depths"]) // 2
    layers = [(f"encode_layers.{i}.", i) for i in range(n)] + [(f"decode_layers{i}.", i + 3) for i in range(n)]
    for pre, li in layers:
        t0 = t
        for b in range(cfg["depths"][li]):
            t = re_block(t, P, f"{pre}residual_group.blocks.{b}.", cfg["num_heads"][li], ws, 0 if b % 2 == 0 else ws // 2, rnd)
        t = rnd(conv(t, pre + "conv") + t0)
    t = ln(t, "norm")
    res = rnd(conv(t, "conv_after_body") + xf)
    return xn + conv(res, "conv_last", ident).permute(0, 3, 1, 2) + mean


def naive_and_truth(fn, x, P, *a, **k):
    """(naive fp32 with bf16 storage points, float64 truth) of a restatement on the CPU"""
    with torch.no_grad():
        naive = fn(x.float(), {n: v.float() for n, v in P.items()}, *a, rnd=rnd_bf16, **k)
        truth = fn(x.double(), {n: v.double() for n, v in P.items()}, *a, rnd=ident, **k)
    return naive, truth


def _cpu_sd(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def _net(cfg, dev, act_dtype="bf16", seed=0):
    from basicsr.archs import build_network

    net = build_network(dict(type="SwinIR", act_dtype=act_dtype, **cfg))
    fill_module_(net, seed=seed)
    return net.to(dev).eval()


def _padded_map(x, dev):
    """a CPU fp32 NCHW tensor as the zero-padded bf16 channels_last device map the kernels take"""
    from basicsr.archs.swinir_arch import pad8

    B, C_, H, W = x.shape
    xp = torch.zeros(B, pad8(C_), H, W)
    xp[:, :C_] = x
    return xp.to(dev).to(BF).contiguous(memory_format=torch.channels_last)


def _pads_bitwise_zero(y, C_):
    pad = y[:, C_:].contiguous()
    return pad.numel() == 0 or bool((pad.view(torch.int16) == 0).all())


def _block(C_, heads, ws, shift, dev, key):
    from basicsr.archs.swinir_arch import SwinTransformerBlock

    blk = SwinTransformerBlock(C_, (128, 128), heads, ws, shift, 2.0)
    blk.load_state_dict({k: keyed_tensor(key + k, tuple(v.shape)) for k, v in blk.state_dict().items()}, strict=True)
    return blk.to(dev).eval()


def _run_block(blk, x, dev):
    from basicsr.archs.swinir_arch import pad8
    from kernel_trace import kernel_trace

    C_ = x.shape[1]
    with torch.no_grad(), kernel_trace() as tr:
        y = blk(_padded_map(x, dev))
        torch.cuda.synchronize()
    assert y.dtype == BF and tuple(y.shape) == (x.shape[0], pad8(C_), x.shape[2], x.shape[3])
    tr.assert_ran("swin_bf16.attn_fwd", "swin_bf16.mlp_fwd", "swin_bf16.wattn_fwd", "swin_bf16.ln_pad_fwd", "nt_bf16.epi_biasgelu.128")
    tr.assert_not_ran(*FP32_SWIN_TAGS)
    assert tr["swin_bf16.attn_fwd"] == tr["swin_bf16.mlp_fwd"] == tr["swin_bf16.wattn_fwd"] == 1 and tr["swin_bf16.ln_pad_fwd"] == 2
    assert tr["nt_bf16.128"] == 4 and tr["nt_bf16.256"] == 0 and tr["nt_bf16.tall512"] == 0, tr.counts
    assert _pads_bitwise_zero(y, C_), "pad columns of y must be bitwise zero"
    return y[:, :C_]


# ---- 1. blocks against the reference's golden vectors ---------------------------------------------------------------------------------------
# c180: M = 192 -- one full and one ragged 128-row tile, windows wrapping in both axes at shift 4
GOLDEN_BLOCKS = [("c180_s0", 180, 6, 8, 0, 1, 8, 24), ("c180_s4", 180, 6, 8, 4, 1, 8, 24),
                 ("c60_ws4_s0", 60, 6, 4, 0, 2, 12, 16), ("c60_ws4_s2", 60, 6, 4, 2, 2, 12, 16)]


@pytest.mark.parametrize("tag,C_,heads,ws,shift,B,H,W", GOLDEN_BLOCKS)
def test_block_vs_golden(dev, golden_dir, tag, C_, heads, ws, shift, B, H, W):
    g = np.load(os.path.join(golden_dir, f"swinir_block_{tag}.npz"))
    blk = _block(C_, heads, ws, shift, dev, f"swb_{tag}.")
    x = keyed_input(f"swb_{tag}.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    y = _run_block(blk, x, dev)
    naive, truth = naive_and_truth(re_block_nchw, x, _cpu_sd(blk), heads, ws, shift)
    assert err(truth, g["y"]) < 1e-5   # the float64 restatement is the reference's arithmetic
    yardstick(f"block {tag}", y, naive, g["y"])


# ---- 2. blocks against float64 at the shapes that stress the new code -----------------------------------------------------------------------
OTHER_BLOCKS = [(180, 6, 8, 4, 2, 16, 24),   # default geometry
                (36, 6, 8, 0, 3, 8, 8),      # hd 6 -> 8, three images inside two row tiles
                (64, 2, 8, 4, 1, 8, 16),     # hd = 32, no padding anywhere
                (64, 1, 4, 2, 2, 12, 8),     # hd = 64, N = 16 < NP: the softmax mask is live
                (56, 2, 7, 3, 1, 14, 21),    # N = 49, hd 28 -> 32
                (40, 1, 5, 1, 1, 10, 5),     # N = 25, hd 40: DP 64 with NP 32
                (96, 2, 6, 5, 1, 12, 6),     # N = 36, hd 48, one window across
                (24, 2, 1, 0, 2, 3, 5),      # N = 1
                (36, 1, 3, 2, 1, 6, 9)]      # N = 9, shift ws - 1


@pytest.mark.parametrize("C_,heads,ws,shift,B,H,W", OTHER_BLOCKS)
def test_block_vs_float64(dev, C_, heads, ws, shift, B, H, W):
    blk = _block(C_, heads, ws, shift, dev, f"swb16_{C_}_{heads}.")
    x = keyed_input(f"swb16_{C_}_{heads}.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    y = _run_block(blk, x, dev)
    naive, truth = naive_and_truth(re_block_nchw, x, _cpu_sd(blk), heads, ws, shift)
    yardstick(f"block C={C_} heads={heads} ws={ws} shift={shift}", y, naive, truth)


# ---- 3. LayerNorm alone -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,Cp,M", [(180, 184, 97), (36, 40, 129), (64, 64, 128)])
def test_layernorm_padded_rows(dev, C_, Cp, M):
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    x = keyed_input(f"swln{C_}.x", (M, Cp), lo=-2.0, hi=2.0).to(BF)       # (the pad columns of the INPUT hold values: they must be ignored)
    w, b = keyed_tensor(f"swln{C_}.w", (C_,)) + 1.0, keyed_tensor(f"swln{C_}.b", (C_,))
    wp, bp = torch.zeros(Cp), torch.zeros(Cp)
    wp[:C_], bp[:C_] = w, b
    xm = x.t().reshape(1, Cp, M, 1).to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), kernel_trace() as tr:
        y = DF.ln_pad_bf16(xm, wp.to(dev), bp.to(dev), C_, 1e-5)
        torch.cuda.synchronize()
    assert tr["swin_bf16.ln_pad_fwd"] == 1 and tr["ln_fwd_bf16"] == 0
    y = y.reshape(Cp, M).t().cpu()
    assert bool((y[:, C_:].contiguous().view(torch.int16) == 0).all()) if Cp > C_ else True
    T = F.layer_norm(x[:, :C_].double(), (C_,), w.double(), b.double(), 1e-5)
    d = (y[:, :C_].double() - T).abs()
    # one bf16 rounding of the result: half an ulp is at most 2^-8 |T|; 4e-6 of the scale for the fp32 arithmetic before it
    bound = 2.0 ** -8 * T.abs() + 4e-6 * float(T.abs().max())
    print(f"LayerNorm {C_}/{Cp} M={M}: max |y - T| {float(d.max()):.3e}, worst ratio to its bound {float((d / bound).max()):.3f}")
    assert bool((d <= bound).all())


# ---- 4. tiny network against the golden vector --------------------------------------------------------------------------------------------------
def test_tiny_net_golden(dev, golden_dir):
    from kernel_trace import kernel_trace

    g = np.load(os.path.join(golden_dir, "swinir_tiny.npz"))
    net = _net(TINY, dev)
    x = keyed_input("swt.x", (2, 3, 32, 40))
    with torch.no_grad(), kernel_trace() as tr:
        y = net(x.to(dev))
        torch.cuda.synchronize()
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(g["y"].shape)
    nblk = sum(TINY["depths"])
    assert tr["swin_bf16.attn_fwd"] == tr["swin_bf16.mlp_fwd"] == tr["swin_bf16.wattn_fwd"] == nblk == 12, tr.counts
    assert tr["swin_bf16.ln_pad_fwd"] == 2 * nblk + 2 and tr["rcan_bf16.res_fwd"] == 7
    tr.assert_not_ran("rcan_bf16.wpack_per_call", *FP32_SWIN_TAGS)
    assert tr["edge.b2s_bf16"] == 1 and tr["edge.s2b_bf16"] == 1   # conv_last on the bf16-input edge kernel, conv_first emitting bf16
    naive, truth = naive_and_truth(re_net, x, _cpu_sd(net), TINY)
    assert err(truth, g["y"]) < 1e-5
    yardstick("tiny net", y, naive, g["y"])
    # the same network object back on the fp32 path: bit-identical to one that was never switched
    net.set_act_dtype("fp32")
    fresh = _net(TINY, dev, act_dtype="fp32")
    with torch.no_grad(), kernel_trace() as tr:
        y32 = net(x.to(dev))
        torch.cuda.synchronize()
    assert tr["swin_wattn_fwd"] == 12 and tr["swin_bf16.attn_fwd"] == 0
    with torch.no_grad():
        assert torch.equal(y32, fresh(x.to(dev)))
    assert err(y32, g["y"]) <= 5e-5


# ---- 5. the default 5D network ------------------------------------------------------------------------------------------------------------------
def test_default_net_golden(dev, golden_dir):
    """the CPU emulation of the 36-block network at the golden file's 64 x 64 input takes a few seconds: the yardstick is used as it stands"""
    g = np.load(os.path.join(golden_dir, "swinir_full.npz"))
    net = _net(FULL, dev)
    assert list(net.state_dict().keys()) == list(g["keys"]) and net.padded_dim() == 184
    x = keyed_input("swf.x", (1, 3, 64, 64))
    with torch.no_grad():
        y = net(x.to(dev))
    naive, truth = naive_and_truth(re_net, x, _cpu_sd(net), FULL)
    assert err(truth[..., ::4, ::4], g["y_sub"]) < 1e-5
    yardstick("default net y_sub", y[..., ::4, ::4], naive[..., ::4, ::4], g["y_sub"])
    # the two scalar entries by the same rule, at the output's scale (T = the golden scalar, the scale max|y_sub|)
    scale = float(np.abs(g["y_sub"]).max())
    for name, f in (("y_mean", lambda t: float(t.double().mean())), ("y_absmean", lambda t: float(t.double().abs().mean()))):
        eh, en = abs(f(y.cpu()) - float(g[name])) / scale, abs(f(naive) - float(g[name])) / scale
        print(f"default net {name}: err(HIP) {eh:.3e}  err(naive) {en:.3e}  bound {1.5 * en + 4e-3:.3e}")
        assert eh <= 1.5 * en + 4e-3


# ---- 6. determinism, batch consistency ----------------------------------------------------------------------------------------------------------
def test_determinism_and_batch_consistency(dev):
    net = _net(TINY, dev)
    x = keyed_input("swb16.batch", (3, 3, 24, 16))   # M = 384 per image: an image boundary inside a 128-row tile of the batch
    with torch.no_grad():
        yb = net(x.to(dev))
        assert torch.equal(net(x.to(dev)), yb), "two runs must agree bit for bit"
        singles = torch.cat([net(x[i:i + 1].to(dev)) for i in range(3)], 0)
    assert bool(torch.isfinite(yb).all())
    assert torch.equal(yb, singles), "a batch of three must equal the three one-image forwards bit for bit"


# ---- 7. exact-size workspaces under red zones ---------------------------------------------------------------------------------------------------
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
    x = _padded_map(keyed_input("swrz.x", (B, C_, H, W), lo=-1.0, hi=1.0), dev)
    blk.refresh_bf16()
    t = blk._swin_bf16.t
    with torch.no_grad():
        ref = [blk(x), DF.ln_pad_bf16(x, t["norm1_w"], t["norm1_b"], C_)]
        with redzone() as rz:
            got = [blk(x), DF.ln_pad_bf16(x, t["norm1_w"], t["norm1_b"], C_)]
        assert rz.count >= 5   # two workspaces, three outputs
    for a, b in zip(ref, got):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    # one byte short: refused before any launch
    pa = _lib.SwinAttnBf16Params(*[t[k].data_ptr() for k in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b")])
    pm = _lib.SwinMlpBf16Params(*[t[k].data_ptr() for k in ("norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")])
    y = torch.empty_like(x)
    st = torch.cuda.current_stream(dev).cuda_stream
    need = [lib.dcpt_swin_attn_bf16_ws_bytes(B, H, W, C_, Cp, heads, hdp, ws), lib.dcpt_swin_mlp_bf16_ws_bytes(B, H, W, C_, Cp, hidden)]
    assert min(need) > 0
    wsb = torch.empty(max(need), dtype=torch.uint8, device=dev)
    with kernel_trace() as tr:
        rcs = [lib.dcpt_swin_attn_fwd_bf16(C.byref(pa), x.data_ptr(), y.data_ptr(), wsb.data_ptr(), need[0] - 1, B, H, W, C_, Cp, heads, hdp, ws,
                                           shift, st),
               lib.dcpt_swin_mlp_fwd_bf16(C.byref(pm), x.data_ptr(), y.data_ptr(), wsb.data_ptr(), need[1] - 1, B, H, W, C_, Cp, hidden, st)]
    assert all(rc != 0 for rc in rcs), rcs
    assert "workspace too small" in lib.dcpt_last_error().decode()
    assert tr.counts == {}, f"a refused call launched: {tr.counts}"


# ---- 8. pack staleness ----------------------------------------------------------------------------------------------------------------------------
def test_pack_staleness(dev):
    from kernel_trace import kernel_trace

    net = _net(TINY, dev)
    x = keyed_input("swpack", (1, 3, 16, 24)).to(dev)
    nsets = 2 + 2 + 12 + 7   # conv_first / conv_last, the two network norms, 12 blocks, 6 RSTB convs + conv_after_body
    with torch.no_grad():
        with kernel_trace() as tr:
            y = net(x)
        assert net.pack_builds == nsets and tr["head.wpack_multi"] == 1
        with kernel_trace() as tr:      # an unchanged network repacks nothing
            assert torch.equal(net(x), y)
        assert net.pack_builds == nsets and tr["head.wpack_multi"] == 0 and tr["rcan_bf16.wpack_per_call"] == 0
        # an in-place edit makes exactly that block's set stale
        net.encode_layers[1].residual_group.blocks[1].attn.qkv.weight.mul_(1.5)
        y_edit = net(x)
        assert net.pack_builds == nsets + 1 and not torch.equal(y_edit, y)
        fresh = _net(TINY, dev)
        fresh.load_state_dict(net.state_dict())
        assert torch.equal(fresh(x), y_edit)
        # ... and an edited conv weight its padded copy and its operand image
        net.decode_layers0.conv.weight.mul_(0.5)
        with kernel_trace() as tr:
            y_conv = net(x)
        assert net.pack_builds == nsets + 2 and tr["head.wpack_multi"] == 1 and not torch.equal(y_conv, y_edit)
        fresh.load_state_dict(net.state_dict())
        assert torch.equal(fresh(x), y_conv)
        # load_state_dict makes every set stale
        sd = {k: (v * 0.5 if k.endswith("mlp.fc2.weight") else v.clone()) for k, v in net.state_dict().items()}
        net.load_state_dict(sd, strict=True)
        y_load = net(x)
        assert net.pack_builds == 2 * nsets + 2 and not torch.equal(y_load, y_conv)
        fresh = _net(TINY, dev)
        fresh.load_state_dict(sd)
        assert torch.equal(fresh(x), y_load)


# ---- 9. SRModel -----------------------------------------------------------------------------------------------------------------------------------
def _srmodel(act_dtype, **extra):
    from basicsr.models import build_model

    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="SwinIR", act_dtype=act_dtype, **TINY), path=dict(pretrain_network_g=None), **extra)
    opt.setdefault("val", dict(save_img=False))
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    return m


def test_srmodel_tiled_inference_equals_tiles_alone(dev):
    """SRModel.test_tile with network_g.act_dtype: bf16: tiles of 16 x 16, 16 x 24, 24 x 16 and 24 x 24 pixels stacked by shape and run on two
    streams; each tile's interior equals the bf16 network run on that padded tile alone, bit for bit"""
    size, pad = 8, 8
    m = _srmodel("bf16", tile=dict(infer_size=size, tile_pad=pad))
    assert m.net_g.act_dtype == "bf16"
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


def test_srmodel_reflect_pad_and_metrics(dev):
    """an image whose sides are no multiples of the window goes through SRModel's reflect padding and comes back at its own size; val.metrics run"""
    from basicsr.data import build_dataloader, build_dataset

    metrics = dict(psnr=dict(type="calculate_psnr", crop_border=0, test_y_channel=False),
                   ssim=dict(type="calculate_ssim", crop_border=0, test_y_channel=False))
    res = {}
    for act in ("bf16", "fp32"):
        m = _srmodel(act, val=dict(save_img=False, metrics=metrics))
        dopt = dict(name="syn", type="SyntheticPairedDataset", phase="val", num=2, size=(21, 19), seed=3)
        loader = build_dataloader(build_dataset(dopt), dopt)
        res[act] = dict(m.nondist_validation(loader, 1, None, False))
        assert m.mod_pad_h == 3 and m.mod_pad_w == 5
        m.feed_data({"lq": keyed_input("swpadimg", (1, 3, 21, 19))})   # (validation drops its images: one more by hand for the size)
        m.pre_test()
        assert tuple(m.lq.shape[-2:]) == (24, 24)
        m.test()
        m.post_test()
        assert tuple(m.output.shape) == (1, 3, 21, 19) and bool(torch.isfinite(m.output).all())
        assert np.isfinite(res[act]["psnr"]) and np.isfinite(res[act]["ssim"])
    print(f"validation metrics: {res}")
    assert abs(res["bf16"]["psnr"] - res["fp32"]["psnr"]) <= 0.5   # the same images restored by the same weights: not a precision claim


# ---- 10. memory -------------------------------------------------------------------------------------------------------------------------------------
def test_memory_below_fp32(dev):
    net = _net(FULL, dev)
    x = keyed_input("swmem", (1, 3, 64, 64)).to(dev)

    def peak(act_dtype):
        net.set_act_dtype(act_dtype)
        with torch.no_grad():
            net(x)   # workspaces (and operand caches) grown
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            y = net(x)
            torch.cuda.synchronize()
            after = torch.cuda.memory_allocated(dev)
            pk = torch.cuda.max_memory_allocated(dev) - before
        assert after - before <= 4 * y.numel() * 4 + (1 << 20), f"{act_dtype} inference kept {after - before} bytes"
        return pk

    p16, p32 = peak("bf16"), peak("fp32")
    print(f"peak above the resident state: bf16 {p16} B, fp32 {p32} B, ratio {p16 / p32:.3f}")
    assert p16 < p32
