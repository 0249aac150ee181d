"""GPU parity: SwinIR (basicsr/archs/swinir_arch.py over dcpt_swin_*, dcpt_conv3x3_res_*, dcpt_img_affine) against the golden vectors of
the real reference (tools/make_golden_swinir.py) and against an independent torch restatement of the reference's arithmetic on the
device, for shapes the fixtures do not hold."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = dict(embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
TINY = dict(embed_dim=36, depths=[2] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
BLOCKS = [("c180_s0", 180, 6, 8, 0, 1, 8, 24), ("c180_s4", 180, 6, 8, 4, 1, 8, 24),
          ("c60_ws4_s0", 60, 6, 4, 0, 2, 12, 16), ("c60_ws4_s2", 60, 6, 4, 2, 2, 12, 16)]
SUB = 29   # tools/make_golden_swinir.py: large gradients are stored as every 29th element


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def check(name, a, b, tol):
    e = relerr(a, b)
    assert np.isfinite(e) and e <= tol, f"{name}: scale-relative max error {e:.3e} > {tol:.1e}"


def check_grads(module, g, tol):
    for k, p in module.named_parameters():
        if "g." + k in g:
            check("grad " + k, p.grad, g["g." + k], tol)
        else:
            check("grad (every 29th) " + k, p.grad.flatten()[::SUB], g["gsub." + k], tol)


def _net(cfg, dev):
    from basicsr.archs import build_network

    net = build_network(dict(type="SwinIR", **cfg))
    fill_module_(net, seed=0)
    return net.to(dev)


# ---- independent restatement of the reference's arithmetic (torch on the device; checker only) ------------------------------------
def ref_block(x, P, pre, heads, ws, shift):
    B, C, H, W = x.shape
    hd = C // heads
    t = x.permute(0, 2, 3, 1)
    h = F.layer_norm(t, (C,), P[pre + "norm1.weight"], P[pre + "norm1.bias"], 1e-5)
    if shift:
        h = torch.roll(h, (-shift, -shift), (1, 2))
    win = h.reshape(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)
    qkv = F.linear(win, P[pre + "attn.qkv.weight"], P[pre + "attn.qkv.bias"]).reshape(win.shape[0], ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * hd ** -0.5, qkv[1], qkv[2]
    o = (torch.softmax(q @ k.transpose(-2, -1), -1) @ v).transpose(1, 2).reshape(-1, ws * ws, C)
    o = F.linear(o, P[pre + "attn.proj.weight"], P[pre + "attn.proj.bias"])
    o = o.reshape(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    t = t + o
    m = F.layer_norm(t, (C,), P[pre + "norm2.weight"], P[pre + "norm2.bias"], 1e-5)
    m = F.linear(F.gelu(F.linear(m, P[pre + "mlp.fc1.weight"], P[pre + "mlp.fc1.bias"])), P[pre + "mlp.fc2.weight"], P[pre + "mlp.fc2.bias"])
    return (t + m).permute(0, 3, 1, 2)


def ref_net(x, P, cfg, img_size=128):
    ws = cfg["window_size"] if img_size > cfg["window_size"] else img_size
    mean = torch.tensor([0.4488, 0.4371, 0.4040], device=x.device).view(1, 3, 1, 1)
    xn = x - mean
    xf = F.conv2d(xn, P["conv_first.weight"], P["conv_first.bias"], padding=1)

    def ln(t, pre):
        return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), P[pre + ".weight"], P[pre + ".bias"], 1e-5).permute(0, 3, 1, 2)

    t = ln(xf, "patch_embed.norm")
    n = len(cfg["depths"]) // 2
    layers = [(f"encode_layers.{i}.", i) for i in range(n)] + [(f"decode_layers{i}.", i + 3) for i in range(n)]
    for pre, li in layers:
        t0 = t
        for b in range(cfg["depths"][li]):
            t = ref_block(t, P, f"{pre}residual_group.blocks.{b}.", cfg["num_heads"][li], ws, 0 if b % 2 == 0 else ws // 2)
        t = F.conv2d(t, P[pre + "conv.weight"], P[pre + "conv.bias"], padding=1) + t0
    t = ln(t, "norm")
    res = F.conv2d(t, P["conv_after_body.weight"], P["conv_after_body.bias"], padding=1) + xf
    return (xn + F.conv2d(res, P["conv_last.weight"], P["conv_last.bias"], padding=1)) + mean


# ---- golden vectors of the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,C,heads,ws,shift,B,H,W", BLOCKS)
def test_block_golden(dev, golden_dir, tag, C, heads, ws, shift, B, H, W):
    from basicsr.archs.swinir_arch import SwinTransformerBlock

    g = np.load(os.path.join(golden_dir, f"swinir_block_{tag}.npz"))
    blk = SwinTransformerBlock(C, (128, 128), heads, ws, shift, 2.0)
    blk.load_state_dict({k: keyed_tensor(f"swb_{tag}." + k, tuple(v.shape)) for k, v in blk.state_dict().items()}, strict=True)
    blk = blk.to(dev)
    x = keyed_input(f"swb_{tag}.x", (B, C, H, W), lo=-1.0, hi=1.0).to(dev).requires_grad_(True)
    go = keyed_input(f"swb_{tag}.go", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
    y = blk(x)
    y.backward(go)
    check("y", y, g["y"], 5e-5)
    check("dx", x.grad, g["dx"], 2e-4)
    check_grads(blk, g, 3e-4)


def test_tiny_net_golden(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "swinir_tiny.npz"))
    net = _net(TINY, dev)
    x = keyed_input("swt.x", (2, 3, 32, 40)).to(dev).requires_grad_(True)
    go = keyed_input("swt.go", (2, 3, 32, 40), lo=-1.0, hi=1.0).to(dev)
    y = net(x)
    y.backward(go)
    check("y", y, g["y"], 5e-5)
    check("dx", x.grad, g["dx"], 2e-4)
    check_grads(net, g, 3e-4)


def test_full_5d_net_golden(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "swinir_full.npz"))
    net = _net(FULL, dev)
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["keys"]) and len(sd) == int(g["n_keys"]) == 454
    assert sum(p.numel() for p in net.parameters()) == int(g["n_params"]) == 11455563
    x = keyed_input("swf.x", (1, 3, 64, 64)).to(dev).requires_grad_(True)
    gt = keyed_input("swf.gt", (1, 3, 64, 64)).to(dev)
    y = net(x)
    loss = (y - gt).abs().mean()
    loss.backward()
    check("y_sub", y[..., ::4, ::4], g["y_sub"], 5e-5)
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    check("dx_sub", x.grad[..., ::4, ::4], g["dx_sub"], 2e-4)
    names = list(g["g_names"])
    assert names == [k for k, _ in net.named_parameters()]
    for i, (k, p) in enumerate(net.named_parameters()):
        gd = p.grad.double()
        l2 = float(gd.pow(2).sum().sqrt())
        assert abs(l2 - g["g_l2"][i]) <= 3e-4 * g["g_l2"][i], f"grad L2 of {k}: {l2} vs {g['g_l2'][i]}"
        assert abs(float(gd.sum()) - g["g_sum"][i]) <= 3e-4 * g["g_abs"][i], f"grad sum of {k}"


# ---- restatement on further shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 128, 128), (1, 72, 136)])
def test_net_vs_restatement(dev, B, H, W):
    net = _net(TINY, dev)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    x = keyed_input(f"swr.x{H}", (B, 3, H, W)).to(dev)
    go = keyed_input(f"swr.go{H}", (B, 3, H, W), lo=-1.0, hi=1.0).to(dev)
    xr = x.clone().requires_grad_(True)
    yr = ref_net(xr, P, TINY)
    yr.backward(go)
    from kernel_trace import kernel_trace

    xg = x.clone().requires_grad_(True)
    with kernel_trace() as tr:
        y = net(xg)
        y.backward(go)
        torch.cuda.synchronize()
    tr.assert_ran("swin_wattn_fwd", "swin_wattn_bwd", "swin_conv3x3_res_fwd", "swin_conv3x3_res_bwd")
    check("y", y, yr, 5e-5)
    check("dx", xg.grad, xr.grad, 2e-4)
    for k, p in net.named_parameters():
        check("grad " + k, p.grad, P[k].grad, 3e-4)


def test_block_vs_restatement_head_dims(dev):
    """head_dim 64 (the 64-column kernel form) and head_dim 3 with a 2 x 2 window, both shifts"""
    from basicsr.archs.swinir_arch import SwinTransformerBlock

    for C, heads, ws, H, W in ((128, 2, 8, 16, 24), (12, 4, 2, 6, 10)):
        for shift in (0, ws // 2):
            blk = SwinTransformerBlock(C, (128, 128), heads, ws, shift, 2.0)
            fill_module_(blk, seed=C + shift)
            blk = blk.to(dev)
            P = {k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
            x = keyed_input(f"swrb{C}", (2, C, H, W), lo=-1.0, hi=1.0).to(dev)
            go = keyed_input(f"swrb{C}.go", (2, C, H, W), lo=-1.0, hi=1.0).to(dev)
            xr, xg = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            yr = ref_block(xr, P, "", heads, ws, shift)
            yr.backward(go)
            y = blk(xg)
            y.backward(go)
            check(f"y C={C} shift={shift}", y, yr, 5e-5)
            check(f"dx C={C} shift={shift}", xg.grad, xr.grad, 2e-4)
            for k, p in blk.named_parameters():
                check(f"grad {k} C={C} shift={shift}", p.grad, P[k].grad, 3e-4)


def test_batch_consistency_and_no_grad_bit_identity(dev):
    net = _net(TINY, dev)
    x = keyed_input("swb.batch", (3, 3, 32, 48)).to(dev)
    with torch.no_grad():
        yb = net(x)
        singles = torch.cat([net(x[i:i + 1]) for i in range(3)], 0)
    check("batched vs one image at a time", yb, singles, 1e-6)
    x.requires_grad_(True)
    yg = net(x)
    assert yg.requires_grad and torch.equal(yg.detach(), yb), "no_grad output must equal the grad-mode output bit for bit"


def test_no_grad_keeps_nothing_for_backward(dev):
    net = _net(TINY, dev).eval()
    x = keyed_input("swb.mem", (2, 3, 64, 64)).to(dev)
    with torch.no_grad():
        net(x)   # workspaces grown
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        y = net(x)
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated(dev)
    assert after - before <= 4 * y.numel() * 4 + (1 << 20), f"inference kept {after - before} bytes"


def test_srmodel_training_step_vs_restatement(dev):
    """one SRModel.optimize_parameters (L1 + the fused AdamW) against the same step of the restatement with torch.optim.AdamW"""
    from basicsr.models import build_model

    lr = 1e-3
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
               network_g=dict(type="SwinIR", **TINY), path=dict(),
               train=dict(pixel_opt=dict(type="L1Loss", loss_weight=1.0, reduction="mean"),
                          optim_g=dict(type="AdamW", lr=lr, weight_decay=0.01, fused=True)))
    m = build_model(opt)
    from dcpt_amd.optim import FusedAdamW

    assert isinstance(m.optimizer_g, FusedAdamW)
    fill_module_(m.net_g, seed=0)
    P0 = {k: v.detach().clone() for k, v in m.net_g.state_dict().items()}
    lq, gt = keyed_input("swstep.lq", (2, 3, 32, 32)), keyed_input("swstep.gt", (2, 3, 32, 32))
    m.feed_data({"lq": lq, "gt": gt})
    m.optimize_parameters(1)
    loss = float(m.log_dict["l_pix"])
    P = {k: v.clone().to(dev).requires_grad_(True) for k, v in P0.items()}
    ref_opt = torch.optim.AdamW(list(P.values()), lr=lr, weight_decay=0.01)
    lr_loss = F.l1_loss(ref_net(lq.to(dev), P, TINY), gt.to(dev))
    lr_loss.backward()
    ref_opt.step()
    assert abs(loss - float(lr_loss)) <= 1e-5 * float(lr_loss), (loss, float(lr_loss))
    for k, p in m.net_g.named_parameters():
        # the first AdamW step is ~lr * sign(g): compare where the gradient stands clear of rounding noise (the key bias of every
        # block has an exactly-zero gradient -- softmax is invariant to it -- so its sign there is noise in both computations)
        g = P[k].grad
        sig = g.abs() > 1e-3 * g.abs().max()
        assert bool((p.detach() - P0[k]).abs().le(1.05 * lr * (1 + 0.01 * P0[k].abs())).all()), k
        if bool(sig.any()):
            check("AdamW update of " + k, (p.detach() - P0[k])[sig], (P[k].detach() - P0[k])[sig], 2e-2)


def test_kernel_trace_reaches_window_kernels(dev):
    from kernel_trace import kernel_trace

    net = _net(TINY, dev)
    x = keyed_input("swtrace", (1, 3, 16, 16)).to(dev).requires_grad_(True)
    with kernel_trace() as tr:
        net(x).sum().backward()
        torch.cuda.synchronize()
    tr.assert_ran("swin_wattn_fwd", "swin_wattn_bwd")
    assert tr["swin_wattn_fwd"] == tr["swin_wattn_bwd"] == 12   # one per Swin block


def test_tiled_inference_equals_untiled_tiles(dev):
    """SRModel.test_tile: each tile's interior equals the network run on that padded tile alone"""
    from basicsr.models import build_model

    size, pad = 32, 8
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="SwinIR", **TINY), path=dict(), tile=dict(infer_size=size, tile_pad=pad), val=dict(save_img=False))
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    img = keyed_input("swtile", (1, 3, 64, 96))
    m.feed_data({"lq": img})
    m.pre_test()
    m.test_tile()
    m.post_test()
    got = m.output.cpu()
    lq = img.to(dev)
    want = torch.zeros_like(img)
    with torch.no_grad():
        for ty in range(2):
            for tx in range(3):
                x0, y0 = tx * size, ty * size
                xp0, yp0, xp1, yp1 = max(x0 - pad, 0), max(y0 - pad, 0), min(x0 + size + pad, 96), min(y0 + size + pad, 64)
                out = m.net_g(lq[:, :, yp0:yp1, xp0:xp1].contiguous())
                want[:, :, y0:y0 + size, x0:x0 + size] = out[:, :, y0 - yp0:y0 - yp0 + size, x0 - xp0:x0 - xp0 + size].cpu()
    check("tiled vs per-tile", got, want, 1e-6)


def test_cli_on_swinir_options():
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "basicsr", "test.py"), "-opt", os.path.join(ROOT, "options", "all_in_one", "test", "test_SwinIR_5d.yml")]

    def run():
        p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        out = p.stdout + p.stderr
        vals = {}
        for chunk in out.split("Validation ")[1:]:
            name = chunk.split()[0]
            for metric, v in re.findall(r"#\s*(psnr|ssim):\s*([-0-9.eE+]+)", chunk[:200]):
                vals[(name, metric)] = float(v)
        return out, vals

    out, vals = run()
    assert {("Rain100L", "psnr"), ("Rain100L", "ssim"), ("CBSD68", "psnr"), ("CBSD68", "ssim")} <= set(vals), out[-1500:]
    for (name, metric), v in vals.items():
        assert (0.0 < v <= 1.0) if metric == "ssim" else (5.0 < v < 80.0), (name, metric, v)
    _, vals2 = run()
    assert vals2 == vals, "two runs of the same option file must report identical metrics"
