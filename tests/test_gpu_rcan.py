"""GPU parity: RCAN (basicsr/archs/rcan_arch.py over dcpt_rcab_*, dcpt_conv3x3_ps_*, dcpt_conv3x3_res_*, dcpt_img_affine) against the golden
vectors of the real reference (tools/make_golden_rcan.py) and against an independent torch restatement of the reference's arithmetic on the
device, for shapes the fixtures do not hold."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor

pytestmark = pytest.mark.gpu
BLOCKS = [("c64_s16", 64, 16, 1.0, 2, 13, 17), ("c32_s4", 32, 4, 1.0, 2, 13, 17), ("c64_s16_rs05", 64, 16, 0.5, 2, 13, 17)]
TINY = dict(num_in_ch=3, num_out_ch=3, num_feat=32, num_group=2, num_block=2)
TINY_LR = (2, 3, 11, 13)
SUB = 29   # tools/make_golden_rcan.py: large gradients are stored as every 29th element
MEAN = (0.4488, 0.4371, 0.4040)


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


def _net(cfg, dev, seed=0):
    from basicsr.archs import build_network

    net = build_network(dict(type="RCAN", **cfg))
    fill_module_(net, seed=seed)
    return net.to(dev)


# ---- independent restatement of the reference's arithmetic (torch on the device; checker only) ------------------------------------
def ref_rcab(x, P, pre, res_scale):
    t = F.conv2d(F.relu(F.conv2d(x, P[pre + "rcab.0.weight"], P[pre + "rcab.0.bias"], padding=1)), P[pre + "rcab.2.weight"], P[pre + "rcab.2.bias"],
                 padding=1)
    a = t.mean((2, 3), keepdim=True)
    a = F.relu(F.conv2d(a, P[pre + "rcab.3.attention.1.weight"], P[pre + "rcab.3.attention.1.bias"]))
    a = torch.sigmoid(F.conv2d(a, P[pre + "rcab.3.attention.3.weight"], P[pre + "rcab.3.attention.3.bias"]))
    return x + res_scale * (t * a)


def ref_net(x, P, cfg, upscale, res_scale=1.0, img_range=255.0):
    mean = torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)
    xf = F.conv2d((x - mean) * img_range, P["conv_first.weight"], P["conv_first.bias"], padding=1)
    t = xf
    for gi in range(cfg["num_group"]):
        t0 = t
        for b in range(cfg["num_block"]):
            t = ref_rcab(t, P, f"body.{gi}.residual_group.{b}.", res_scale)
        t = F.conv2d(t, P[f"body.{gi}.conv.weight"], P[f"body.{gi}.conv.bias"], padding=1) + t0
    t = F.conv2d(t, P["conv_after_body.weight"], P["conv_after_body.bias"], padding=1) + xf
    stages = [2] * (upscale.bit_length() - 1) if upscale & (upscale - 1) == 0 else [3]
    for i, r in enumerate(stages):
        t = F.pixel_shuffle(F.conv2d(t, P[f"upsample.{2 * i}.weight"], P[f"upsample.{2 * i}.bias"], padding=1), r)
    return F.conv2d(t, P["conv_last.weight"], P["conv_last.bias"], padding=1) / img_range + mean


# ---- golden vectors of the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,C,sq,rs,B,H,W", BLOCKS)
def test_block_golden(dev, golden_dir, tag, C, sq, rs, B, H, W):
    from basicsr.archs.rcan_arch import RCAB

    g = np.load(os.path.join(golden_dir, f"rcan_block_{tag}.npz"))
    blk = RCAB(C, sq, rs)
    blk.load_state_dict({k: keyed_tensor(f"rcab_{tag}." + k, tuple(v.shape)) for k, v in blk.state_dict().items()}, strict=True)
    blk = blk.to(dev)
    x = keyed_input(f"rcab_{tag}.x", (B, C, H, W), lo=-1.0, hi=1.0).to(dev).requires_grad_(True)
    go = keyed_input(f"rcab_{tag}.go", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
    y = blk(x)
    y.backward(go)
    check("y", y, g["y"], 5e-5)
    check("dx", x.grad, g["dx"], 2e-4)
    check_grads(blk, g, 3e-4)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_tiny_net_golden(dev, golden_dir, s):
    g = np.load(os.path.join(golden_dir, f"rcan_tiny_x{s}.npz"))
    net = _net(dict(TINY, upscale=s), dev)
    B, Cin, h, w = TINY_LR
    x = keyed_input(f"rcant{s}.x", TINY_LR).to(dev).requires_grad_(True)
    go = keyed_input(f"rcant{s}.go", (B, Cin, s * h, s * w), lo=-1.0, hi=1.0).to(dev)
    y = net(x)
    y.backward(go)
    check("y", y, g["y"], 5e-5)
    check("dx", x.grad, g["dx"], 2e-4)
    check_grads(net, g, 3e-4)


def test_default_net_golden(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "rcan_full.npz"))
    net = _net(dict(num_in_ch=3, num_out_ch=3), dev)
    with torch.no_grad():   # tools/make_golden_rcan.py damp_: every RCAB's second conv x 0.1 keeps 160 blocks well conditioned in fp32
        for k, p in net.named_parameters():
            if ".rcab.2." in k:
                p.mul_(0.1)
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["keys"]) and len(sd) == int(g["n_keys"]) == 1310
    x = keyed_input("rcanf.x", (1, 3, 12, 12)).to(dev).requires_grad_(True)
    gt = keyed_input("rcanf.gt", (1, 3, 48, 48)).to(dev)
    y = net(x)
    loss = (y - gt).abs().mean()
    loss.backward()
    check("y_sub", y[..., ::4, ::4], g["y_sub"], 5e-5)
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    check("dx_sub", x.grad[..., ::2, ::2], g["dx_sub"], 2e-4)
    assert list(g["g_names"]) == [k for k, _ in net.named_parameters()]
    for i, (k, p) in enumerate(net.named_parameters()):
        gd = p.grad.double()
        l2 = float(gd.pow(2).sum().sqrt())
        assert abs(l2 - g["g_l2"][i]) <= 3e-4 * g["g_l2"][i], f"grad L2 of {k}: {l2} vs {g['g_l2'][i]}"
        assert abs(float(gd.sum()) - g["g_sum"][i]) <= 3e-4 * g["g_abs"][i], f"grad sum of {k}"


# ---- restatement on further shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,B,h,w", [(4, 3, 9, 7), (3, 3, 16, 24), (2, 1, 40, 33)])
def test_net_vs_restatement(dev, s, B, h, w):
    cfg = dict(TINY, upscale=s, squeeze_factor=8, res_scale=0.7)
    net = _net(cfg, dev, seed=s)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    x = keyed_input(f"rcanr.x{s}", (B, 3, h, w)).to(dev)
    go = keyed_input(f"rcanr.go{s}", (B, 3, s * h, s * w), lo=-1.0, hi=1.0).to(dev)
    xr = x.clone().requires_grad_(True)
    yr = ref_net(xr, P, cfg, s, res_scale=0.7)
    yr.backward(go)
    xg = x.clone().requires_grad_(True)
    y = net(xg)
    y.backward(go)
    check("y", y, yr, 5e-5)
    check("dx", xg.grad, xr.grad, 2e-4)
    for k, p in net.named_parameters():
        check("grad " + k, p.grad, P[k].grad, 3e-4)


def test_block_vs_restatement_wide_and_narrow(dev):
    """C = 128 (two column tiles' worth of images per tile at 5 x 6), C = 12 with Cr = 1, and a map smaller than one GEMM tile"""
    from basicsr.archs.rcan_arch import RCAB

    for C, sq, B, H, W in ((128, 16, 3, 5, 6), (12, 12, 4, 7, 9), (64, 16, 5, 31, 29)):
        blk = RCAB(C, sq, 0.5)
        fill_module_(blk, seed=C)
        blk = blk.to(dev)
        P = {k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
        x = keyed_input(f"rcanb{C}", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
        go = keyed_input(f"rcanb{C}.go", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
        xr, xg = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        yr = ref_rcab(xr, P, "", 0.5)
        yr.backward(go)
        y = blk(xg)
        y.backward(go)
        check(f"y C={C}", y, yr, 5e-5)
        check(f"dx C={C}", xg.grad, xr.grad, 2e-4)
        for k, p in blk.named_parameters():
            check(f"grad {k} C={C}", p.grad, P[k].grad, 3e-4)


def test_batch_consistency_and_no_grad_bit_identity(dev):
    net = _net(dict(TINY, upscale=3), dev)
    x = keyed_input("rcanbatch", (3, 3, 13, 10)).to(dev)
    with torch.no_grad():
        yb = net(x)
        singles = torch.cat([net(x[i:i + 1]) for i in range(3)], 0)
    check("batched vs one image at a time", yb, singles, 1e-6)
    x.requires_grad_(True)
    yg = net(x)
    assert yg.requires_grad and torch.equal(yg.detach(), yb), "no_grad output must equal the grad-mode output bit for bit"
    with torch.no_grad():
        assert torch.equal(net(x), yb), "two runs must agree bit for bit"


def test_no_grad_keeps_nothing_for_backward(dev):
    net = _net(dict(TINY, upscale=4), dev).eval()
    x = keyed_input("rcanmem", (2, 3, 32, 32)).to(dev)
    with torch.no_grad():
        net(x)   # workspaces grown
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        y = net(x)
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated(dev)
    assert after - before <= 4 * y.numel() * 4 + (1 << 20), f"inference kept {after - before} bytes"


def test_backward_is_deterministic(dev):
    net = _net(dict(TINY, upscale=2), dev)
    x = keyed_input("rcandet", (2, 3, 20, 17)).to(dev)
    grads = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        net(x).square().mean().backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_kernel_trace_counts(dev):
    from kernel_trace import kernel_trace

    net = _net(dict(TINY, upscale=4), dev)
    x = keyed_input("rcantrace", (1, 3, 8, 8)).to(dev).requires_grad_(True)
    with kernel_trace() as tr:
        net(x).sum().backward()
        torch.cuda.synchronize()
    assert tr["rcan_rcab_fwd"] == tr["rcan_rcab_bwd"] == 4   # one per RCAB: 2 groups x 2 blocks
    assert tr["rcan_ps_fwd"] == tr["rcan_ps_bwd"] == 2       # one per Upsample stage at x4


def test_srmodel_training_step_vs_restatement(dev):
    """one SRModel.optimize_parameters at scale 4 (L1 + the fused AdamW) against the same step of the restatement with torch.optim.AdamW"""
    from basicsr.models import build_model

    lr = 1e-3
    cfg = dict(TINY, upscale=4)
    opt = dict(name="t", model_type="SRModel", scale=4, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
               network_g=dict(type="RCAN", **cfg), path=dict(),
               train=dict(pixel_opt=dict(type="L1Loss", loss_weight=1.0, reduction="mean"),
                          optim_g=dict(type="AdamW", lr=lr, weight_decay=0.01, fused=True)))
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    P0 = {k: v.detach().clone() for k, v in m.net_g.state_dict().items()}
    lq, gt = keyed_input("rcanstep.lq", (2, 3, 12, 12)), keyed_input("rcanstep.gt", (2, 3, 48, 48))
    m.feed_data({"lq": lq, "gt": gt})
    m.optimize_parameters(1)
    loss = float(m.log_dict["l_pix"])
    P = {k: v.clone().to(dev).requires_grad_(True) for k, v in P0.items()}
    ref_opt = torch.optim.AdamW(list(P.values()), lr=lr, weight_decay=0.01)
    lr_loss = F.l1_loss(ref_net(lq.to(dev), P, cfg, 4), gt.to(dev))
    lr_loss.backward()
    ref_opt.step()
    assert abs(loss - float(lr_loss)) <= 1e-5 * float(lr_loss), (loss, float(lr_loss))
    for k, p in m.net_g.named_parameters():
        g = P[k].grad
        sig = g.abs() > 1e-3 * g.abs().max()
        assert bool((p.detach() - P0[k]).abs().le(1.05 * lr * (1 + 0.01 * P0[k].abs())).all()), k
        if bool(sig.any()):
            check("AdamW update of " + k, (p.detach() - P0[k])[sig], (P[k].detach() - P0[k])[sig], 2e-2)


def test_tiled_inference_equals_untiled_tiles(dev):
    """SRModel.test_tile at scale 4: each tile's interior equals the network run on that padded tile alone"""
    from basicsr.models import build_model

    size, pad, s = 16, 4, 4
    opt = dict(name="t", model_type="SRModel", scale=s, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="RCAN", **dict(TINY, upscale=s)), path=dict(), tile=dict(infer_size=size, tile_pad=pad),
               val=dict(save_img=False))
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    img = keyed_input("rcantile", (1, 3, 32, 48))
    m.feed_data({"lq": img})
    m.pre_test()
    m.test_tile()
    m.post_test()
    got = m.output.cpu()
    assert tuple(got.shape) == (1, 3, 128, 192)
    lq = img.to(dev)
    want = torch.zeros_like(got)
    with torch.no_grad():
        for ty in range(2):
            for tx in range(3):
                x0, y0 = tx * size, ty * size
                xp0, yp0, xp1, yp1 = max(x0 - pad, 0), max(y0 - pad, 0), min(x0 + size + pad, 48), min(y0 + size + pad, 32)
                out = m.net_g(lq[:, :, yp0:yp1, xp0:xp1].contiguous())
                oy, ox = s * (y0 - yp0), s * (x0 - xp0)
                want[:, :, s * y0:s * (y0 + size), s * x0:s * (x0 + size)] = out[:, :, oy:oy + s * size, ox:ox + s * size].cpu()
    check("tiled vs per-tile", got, want, 1e-6)
