"""Shared by the bf16_res32 tests (RCAN / SwinIR on bf16 maps around an fp32 residual stream): the project's yardstick for bf16 storage and
the kernel-blind CPU restatements of tests/test_gpu_rcan_bf16.py / tests/test_gpu_swinir_bf16.py with a SECOND rounding argument:
    rnd   the rounding of every bf16 storage point (weight operand images, h, t, LN output, qkv, P, attention output, GELU output, the maps
          after the stream's end), torch.bfloat16 in the naive emulation and the identity in the float64 truth;
    srnd  the rounding of the RESIDUAL STREAM where it is stored.  The identity for "bf16_res32"; ``rnd`` itself gives the "bf16" mode's
          restatement back (rounding twice is rounding once).
The convs read rnd(stream): every GEMM operand is bf16 in both modes.  Nothing here knows of padding or of a kernel."""
import numpy as np
import torch
import torch.nn.functional as F

BF = torch.bfloat16
MEAN = (0.4488, 0.4371, 0.4040)


def _np(a):
    return a.detach().float().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def err(a, T):
    a, T = _np(a), _np(T)
    assert a.shape == T.shape, (a.shape, T.shape)
    return float(np.abs(a - T).max() / max(1e-12, np.abs(T).max()))


def yardstick(name, hip, naive, T):
    """err(HIP) <= 1.5 err(naive) + 4e-3 (one bf16 ulp at the tensor's scale; 1.5 for the spread of a max-norm); prints the three numbers"""
    eh, en = err(hip, T), err(naive, T)
    print(f"{name}: err(HIP) {eh:.3e}  err(naive) {en:.3e}  bound {1.5 * en + 4e-3:.3e}")
    assert np.isfinite(eh) and eh <= 1.5 * en + 4e-3, f"{name}: err(HIP) {eh:.3e} > 1.5 * err(naive) {en:.3e} + 4e-3"
    return eh


def rnd_bf16(t):
    return t.to(BF).to(t.dtype)


def ident(t):
    return t


def naive_and_truth(fn, x, P, *a, **k):
    """(naive fp32 emulation of bf16_res32: bf16 storage points, unrounded stream;  float64 truth) on the CPU"""
    with torch.no_grad():
        naive = fn(x.float(), {n: v.float() for n, v in P.items()}, *a, rnd=rnd_bf16, srnd=ident, **k)
        truth = fn(x.double(), {n: v.double() for n, v in P.items()}, *a, rnd=ident, srnd=ident, **k)
    return naive, truth


def cpu_sd(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


# ---- RCAN ------------------------------------------------------------------------------------------------------------------------------------
def rcan_rcab(s, P, pre, res_scale, rnd, srnd):
    """s: the stream as stored"""
    h = rnd(F.relu(F.conv2d(rnd(s), rnd(P[pre + "rcab.0.weight"]), P[pre + "rcab.0.bias"], padding=1)))
    tf = F.conv2d(h, rnd(P[pre + "rcab.2.weight"]), P[pre + "rcab.2.bias"], padding=1)
    a = tf.mean((2, 3), keepdim=True)   # of the values before their rounding
    a = F.relu(F.conv2d(a, P[pre + "rcab.3.attention.1.weight"], P[pre + "rcab.3.attention.1.bias"]))
    a = torch.sigmoid(F.conv2d(a, P[pre + "rcab.3.attention.3.weight"], P[pre + "rcab.3.attention.3.bias"]))
    return srnd(s + res_scale * (rnd(tf) * a))


def rcan_net(x, P, cfg, upscale, rnd, srnd, res_scale=1.0, img_range=255.0):
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    xf = srnd(F.conv2d((x - mean) * img_range, P["conv_first.weight"], P["conv_first.bias"], padding=1))
    t = xf
    for gi in range(cfg.get("num_group", 10)):
        t0 = t
        for b in range(cfg.get("num_block", 16)):
            t = rcan_rcab(t, P, f"body.{gi}.residual_group.{b}.", res_scale, rnd, srnd)
        t = srnd(F.conv2d(rnd(t), rnd(P[f"body.{gi}.conv.weight"]), P[f"body.{gi}.conv.bias"], padding=1) + t0)
    t = rnd(F.conv2d(rnd(t), rnd(P["conv_after_body.weight"]), P["conv_after_body.bias"], padding=1) + xf)   # the stream ends here
    stages = [2] * (upscale.bit_length() - 1) if upscale & (upscale - 1) == 0 else [3]
    for i, r in enumerate(stages):
        t = rnd(F.pixel_shuffle(F.conv2d(t, rnd(P[f"upsample.{2 * i}.weight"]), P[f"upsample.{2 * i}.bias"], padding=1), r))
    return F.conv2d(t, P["conv_last.weight"], P["conv_last.bias"], padding=1) / img_range + mean


# ---- SwinIR (unpadded: the C real channels) --------------------------------------------------------------------------------------------------
def swin_attn_half(s, P, pre, heads, ws, shift, rnd, srnd):
    B, H, W, C_ = s.shape
    hd = C_ // heads
    h = rnd(F.layer_norm(s, (C_,), P[pre + "norm1.weight"], P[pre + "norm1.bias"], 1e-5))   # (the LayerNorm reads the stream as stored)
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
    return srnd(s + o)


def swin_mlp_half(t, P, pre, rnd, srnd):
    C_ = t.shape[-1]
    m = rnd(F.layer_norm(t, (C_,), P[pre + "norm2.weight"], P[pre + "norm2.bias"], 1e-5))
    g = rnd(F.gelu(F.linear(m, rnd(P[pre + "mlp.fc1.weight"]), P[pre + "mlp.fc1.bias"])))
    return srnd(t + F.linear(g, rnd(P[pre + "mlp.fc2.weight"]), P[pre + "mlp.fc2.bias"]))


def swin_block(s, P, pre, heads, ws, shift, rnd, srnd):
    """s (B, H, W, C): the stream as stored"""
    return swin_mlp_half(swin_attn_half(s, P, pre, heads, ws, shift, rnd, srnd), P, pre, rnd, srnd)


def swin_block_nchw(x, P, heads, ws, shift, rnd, srnd):
    return swin_block(srnd(x.permute(0, 2, 3, 1)), P, "", heads, ws, shift, rnd, srnd).permute(0, 3, 1, 2)


def swin_net(x, P, cfg, rnd, srnd):
    ws = cfg["window_size"]
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    xn = x - mean

    def conv(t, pre, r=rnd):   # NHWC in / out; r: the rounding of the weight operand image (the edge convs read fp32 weights)
        return F.conv2d(t.permute(0, 3, 1, 2), r(P[pre + ".weight"]), P[pre + ".bias"], padding=1).permute(0, 2, 3, 1)

    def ln(t, pre):
        return rnd(F.layer_norm(t, (t.shape[-1],), P[pre + ".weight"], P[pre + ".bias"], 1e-5))

    xf = srnd(conv(xn.permute(0, 2, 3, 1), "conv_first", ident))
    t = ln(xf, "patch_embed.norm")   # a LayerNorm output is a bf16 storage point: the stream starts from that value
    n = len(cfg["depths"]) // 2
    layers = [(f"encode_layers.{i}.", i) for i in range(n)] + [(f"decode_layers{i}.", i + 3) for i in range(n)]
    for pre, li in layers:
        t0 = t
        for b in range(cfg["depths"][li]):
            t = swin_block(t, P, f"{pre}residual_group.blocks.{b}.", cfg["num_heads"][li], ws, 0 if b % 2 == 0 else ws // 2, rnd, srnd)
        t = srnd(conv(rnd(t), pre + "conv") + t0)
    t = ln(t, "norm")
    res = rnd(conv(t, "conv_after_body") + xf)   # the stream ends here
    return xn + conv(res, "conv_last", ident).permute(0, 3, 1, 2) + mean
