"""GPU parity: SwinIR's super-resolution forms and the 3conv residual (basicsr/archs/swinir_arch.py over dcpt_conv3x3_act_*,
dcpt_up2_conv3x3_act_*, dcpt_conv3x3_ps_out_*, dcpt_conv3conv_res_*, dcpt_conv3x3_ps_*, dcpt_conv3x3_out_*) against the golden vectors of
the real reference (tools/make_golden_swinir_sr.py) and against an independent torch restatement of the reference's arithmetic on the
device, for shapes the fixtures do not hold.  Tolerances are those of test_gpu_swinir.py / test_gpu_rcan.py for the same GEMM families:
scale-relative max error y <= 5e-5, dx <= 2e-4, parameter gradients <= 3e-4."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor
from redzone import redzone
from tests import test_gpu_swinir as TSW
from tests.test_gpu_swinir import check, check_grads

pytestmark = pytest.mark.gpu
TINY = dict(TSW.TINY, img_size=64)
TAGS = {"pixelshuffle": "pixelshuffle", "pixelshuffledirect": "direct", "nearest+conv": "nearestconv"}
# tools/make_golden_swinir_sr.py TINY_NETS: (upsampler, upscale, resi_connection, embed_dim, (H, W))
TINY_NETS = [("pixelshuffle", 2, "1conv", 36, (16, 24)), ("pixelshuffle", 3, "1conv", 36, (16, 16)), ("pixelshuffle", 4, "1conv", 36, (16, 16)),
             ("pixelshuffledirect", 2, "1conv", 36, (16, 24)), ("pixelshuffledirect", 3, "1conv", 36, (16, 16)),
             ("pixelshuffledirect", 4, "1conv", 36, (16, 16)),
             ("nearest+conv", 2, "1conv", 36, (16, 24)), ("nearest+conv", 4, "1conv", 36, (16, 16)),
             ("nearest+conv", 4, "3conv", 48, (16, 16))]
Y_TOL, DX_TOL, G_TOL = 5e-5, 2e-4, 3e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


def _cfg(upsampler, r, resi="1conv", embed=36):
    return dict(TINY, embed_dim=embed, upscale=r, upsampler=upsampler, resi_connection=resi)


def _net(cfg, dev, seed=0):
    from basicsr.archs import build_network

    net = build_network(dict(type="SwinIR", **cfg))
    fill_module_(net, seed=seed)
    return net.to(dev)


# ---- independent restatement of the reference's arithmetic (torch on the device; checker only) ------------------------------------
def ref_conv(t, P, pre, slope=None):
    t = F.conv2d(t, P[pre + ".weight"], P[pre + ".bias"], padding=P[pre + ".weight"].shape[-1] // 2)
    return t if slope is None else F.leaky_relu(t, slope)


def ref_residual_conv(t, P, pre, res):
    if pre + ".weight" in P:
        return ref_conv(t, P, pre) + res
    return ref_conv(ref_conv(ref_conv(t, P, pre + ".0", 0.2), P, pre + ".2", 0.2), P, pre + ".4") + res


def ref_sr_net(x, P, cfg):
    """swinir_arch.py:1061-1100: the SR branches add no image residual and leave the output in the normalised range"""
    ws = cfg["window_size"]
    mean = torch.tensor([0.4488, 0.4371, 0.4040], device=x.device).view(1, 3, 1, 1)
    xf = ref_conv(x - mean, P, "conv_first")

    def ln(t, pre):
        return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), P[pre + ".weight"], P[pre + ".bias"], 1e-5).permute(0, 3, 1, 2)

    t = ln(xf, "patch_embed.norm")
    n = len(cfg["depths"]) // 2
    for pre, li in [(f"encode_layers.{i}.", i) for i in range(n)] + [(f"decode_layers{i}.", i + 3) for i in range(n)]:
        t0 = t
        for b in range(cfg["depths"][li]):
            t = TSW.ref_block(t, P, f"{pre}residual_group.blocks.{b}.", cfg["num_heads"][li], ws, 0 if b % 2 == 0 else ws // 2)
        t = ref_residual_conv(t, P, pre + "conv", t0)
    t = ref_residual_conv(ln(t, "norm"), P, "conv_after_body", xf)
    up, r = cfg["upsampler"], cfg["upscale"]
    if up == "pixelshuffledirect":
        return F.pixel_shuffle(ref_conv(t, P, "upsample.0"), r)
    t = ref_conv(t, P, "conv_before_upsample.0", 0.01)
    if up == "pixelshuffle":
        stages = [2] * (r.bit_length() - 1) if r & (r - 1) == 0 else [3]
        for i, s in enumerate(stages):
            t = F.pixel_shuffle(ref_conv(t, P, f"upsample.{2 * i}"), s)
    else:
        t = ref_conv(F.interpolate(t, scale_factor=2, mode="nearest"), P, "conv_up1", 0.2)
        if r == 4:
            t = ref_conv(F.interpolate(t, scale_factor=2, mode="nearest"), P, "conv_up2", 0.2)
        t = ref_conv(t, P, "conv_hr", 0.2)
    return ref_conv(t, P, "conv_last")


def _run(fn, ref, x, ps, go_shape, tag, dev):
    """y, dx and parameter gradients of the node ``fn(x, *ps)`` against ``ref(x, *ps)``; returns both gradient lists"""
    x = x.to(dev)
    ps = [p.to(dev) for p in ps]
    xg, xr = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    pg, pr = [p.clone().requires_grad_(True) for p in ps], [p.clone().requires_grad_(True) for p in ps]
    y, yr = fn(xg, *pg), ref(xr, *pr)
    assert tuple(y.shape) == tuple(yr.shape) == tuple(go_shape)
    go = keyed_input(tag + ".go", tuple(go_shape), lo=-1.0, hi=1.0).to(dev)
    y.backward(go)
    yr.backward(go)
    check(tag + " y", y, yr, Y_TOL)
    check(tag + " dx", xg.grad, xr.grad, DX_TOL)
    for i, (a, b) in enumerate(zip(pg, pr)):
        check(f"{tag} grad of parameter {i}", a.grad, b.grad, G_TOL)
    return [xg.grad] + [p.grad for p in pg], [xr.grad] + [p.grad for p in pr]


def _act_case(dev, Cin, Cout, B, H, W, slope, up2):
    from dcpt_amd import functional as DF

    tag = f"sract{Cin}_{Cout}_{B}_{H}_{W}_{int(up2)}"
    x = keyed_input(tag + ".x", (B, Cin, H, W), lo=-1.0, hi=1.0)
    ps = [keyed_tensor(tag + ".w", (Cout, Cin, 3, 3)), keyed_tensor(tag + ".b", (Cout,))]
    s = 2 if up2 else 1
    if up2:
        fn = lambda x, w, b: DF.up2_conv3x3_act(x, w, b, slope)   # noqa: E731
        ref = lambda x, w, b: F.leaky_relu(F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1), slope)   # noqa: E731
    else:
        fn = lambda x, w, b: DF.conv3x3_act(x, w, b, slope)   # noqa: E731
        ref = lambda x, w, b: F.leaky_relu(F.conv2d(x, w, b, padding=1), slope)   # noqa: E731
    return _run(fn, ref, x, ps, (B, Cout, s * H, s * W), tag, dev)


def _psout_case(dev, C, Cimg, r, B, H, W):
    from dcpt_amd import functional as DF

    tag = f"srps{C}_{Cimg}_{r}_{B}_{H}_{W}"
    x = keyed_input(tag + ".x", (B, C, H, W), lo=-1.0, hi=1.0)
    ps = [keyed_tensor(tag + ".w", (r * r * Cimg, C, 3, 3)), keyed_tensor(tag + ".b", (r * r * Cimg,))]
    return _run(lambda x, w, b: DF.conv3x3_ps_out(x, w, b, r), lambda x, w, b: F.pixel_shuffle(F.conv2d(x, w, b, padding=1), r), x, ps,
                (B, Cimg, r * H, r * W), tag, dev)


def _c3_case(dev, C, B, H, W):
    from dcpt_amd import functional as DF

    tag = f"src3_{C}_{B}_{H}_{W}"
    Cq = C // 4
    x = keyed_input(tag + ".x", (B, C, H, W), lo=-1.0, hi=1.0)
    ps = [keyed_input(tag + ".res", (B, C, H, W), lo=-1.0, hi=1.0), keyed_tensor(tag + ".w1", (Cq, C, 3, 3)), keyed_tensor(tag + ".b1", (Cq,)),
          keyed_tensor(tag + ".w2", (Cq, Cq, 1, 1)), keyed_tensor(tag + ".b2", (Cq,)), keyed_tensor(tag + ".w3", (C, Cq, 3, 3)),
          keyed_tensor(tag + ".b3", (C,))]

    def ref(x, res, w1, b1, w2, b2, w3, b3):
        return res + F.conv2d(F.leaky_relu(F.conv2d(F.leaky_relu(F.conv2d(x, w1, b1, padding=1), 0.2), w2, b2), 0.2), w3, b3, padding=1)

    return _run(lambda x, res, *p: DF.conv3conv_res(x, *p, res), ref, x, ps, (B, C, H, W), tag, dev)


# ---- golden vectors of the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upsampler,r,resi,embed,hw", TINY_NETS)
def test_tiny_net_golden(dev, golden_dir, upsampler, r, resi, embed, hw):
    tag = f"swinir_sr_{TAGS[upsampler]}_x{r}" + ("_3conv" if resi == "3conv" else "")
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    net = _net(_cfg(upsampler, r, resi, embed), dev)
    H, W = hw
    x = keyed_input(tag + ".x", (2, 3, H, W)).to(dev).requires_grad_(True)
    go = keyed_input(tag + ".go", (2, 3, r * H, r * W), lo=-1.0, hi=1.0).to(dev)
    y = net(x)
    assert tuple(y.shape) == (2, 3, r * H, r * W)
    y.backward(go)
    check("y", y, g["y"], Y_TOL)
    check("dx", x.grad, g["dx"], DX_TOL)
    check_grads(net, g, G_TOL)


@pytest.mark.parametrize("tag,kw", [("classical_x4_c180", dict(embed_dim=180, num_heads=[6] * 6, upsampler="pixelshuffle", upscale=4)),
                                    ("lightweight_x2_c60", dict(embed_dim=60, num_heads=[6] * 6, upsampler="pixelshuffledirect", upscale=2)),
                                    ("realworld_x4_c240_3conv", dict(embed_dim=240, num_heads=[8] * 6, upsampler="nearest+conv", upscale=4,
                                                                     resi_connection="3conv"))])
def test_key_net_forward_golden(dev, golden_dir, tag, kw):
    g = np.load(os.path.join(golden_dir, f"swinir_sr_key_{tag}.npz"))
    net = _net(dict(img_size=64, window_size=8, mlp_ratio=2.0, depths=[6] * 6, **kw), dev)
    with torch.no_grad():
        y = net(keyed_input(f"swinir_sr_key_{tag}.x", (1, 3, 16, 16)).to(dev))
    assert tuple(y.shape) == (1, 3, 16 * kw["upscale"], 16 * kw["upscale"])
    check("y_sub", y[..., ::2, ::2], g["y_sub"], Y_TOL)


# ---- each node alone against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,Cout,B,H,W,slope", [(180, 64, 1, 13, 9, 0.01), (64, 180, 3, 13, 9, 0.2), (64, 64, 2, 16, 24, 1.0),
                                                  (8, 12, 3, 21, 19, 0.2)])
def test_conv3x3_act_vs_restatement(dev, Cin, Cout, B, H, W, slope):
    """M = 117 / 351 / 768 / 1197: not a multiple of 128 or 256 but for one; Cin != Cout both ways; slope 1 = the plain biased conv"""
    _act_case(dev, Cin, Cout, B, H, W, slope, False)


@pytest.mark.parametrize("C,B,H,W", [(64, 1, 13, 9), (64, 3, 13, 9), (36, 2, 8, 12), (8, 3, 1, 1), (16, 1, 1, 5)])
def test_up2_conv3x3_act_vs_restatement(dev, C, B, H, W):
    """odd H / W, one-pixel and one-row sources (every tap of the 2 x 2 output lands on the padding or on the same source pixel)"""
    _act_case(dev, C, C, B, H, W, 0.2, True)


@pytest.mark.parametrize("C,Cimg,r,B,H,W", [(60, 3, 3, 1, 13, 9), (60, 3, 2, 3, 13, 9), (64, 3, 4, 2, 16, 24), (36, 1, 3, 3, 7, 5), (16, 4, 2, 1, 9, 13)])
def test_conv3x3_ps_out_vs_restatement(dev, C, Cimg, r, B, H, W):
    """N = 27 / 12 / 48 / 9 / 16 GEMM columns: r = 3 pads the weight rows to the next multiple of 4"""
    _psout_case(dev, C, Cimg, r, B, H, W)


@pytest.mark.parametrize("C,B,H,W", [(48, 1, 13, 9), (240, 3, 13, 9), (64, 2, 16, 24), (16, 3, 5, 7)])
def test_conv3conv_res_vs_restatement(dev, C, B, H, W):
    _c3_case(dev, C, B, H, W)


def test_classical_upsample_stage_at_64_channels_r3(dev):
    """the existing dcpt_conv3x3_ps stage as SwinIR uses it: num_feat 64, r = 3 (RCAN's tests hold it at 32)"""
    from dcpt_amd import functional as DF

    tag = "srps64r3"
    x = keyed_input(tag + ".x", (1, 64, 13, 9), lo=-1.0, hi=1.0)
    ps = [keyed_tensor(tag + ".w", (576, 64, 3, 3)), keyed_tensor(tag + ".b", (576,))]
    _run(lambda x, w, b: DF.conv3x3_ps(x, w, b, 3), lambda x, w, b: F.pixel_shuffle(F.conv2d(x, w, b, padding=1), 3), x, ps, (1, 64, 39, 27), tag, dev)


# ---- LeakyReLU at exactly zero ----------------------------------------------------------------------------------------------------------
def test_leaky_relu_gradient_at_zero_and_below(dev):
    """output channel 0 has zero weights and zero bias (pre-activation exactly 0 everywhere: torch's backward takes the slope branch there),
    channel 1 zero weights and a negative bias (negative everywhere): bias and weight gradients of those channels equal torch's"""
    from dcpt_amd import functional as DF

    B, C, H, W, slope = 2, 16, 9, 7, 0.2
    x = keyed_input("srzero.x", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
    w = keyed_tensor("srzero.w", (C, C, 3, 3)).to(dev)
    b = keyed_tensor("srzero.b", (C,)).to(dev)
    w[0:2] = 0.0
    b[0], b[1] = 0.0, -0.25
    for up2 in (False, True):
        s = 2 if up2 else 1
        go = keyed_input(f"srzero.go{s}", (B, C, s * H, s * W), lo=-1.0, hi=1.0).to(dev)
        leaves = [[t.clone().requires_grad_(True) for t in (x, w, b)] for _ in range(2)]
        xs = F.interpolate(leaves[1][0], scale_factor=2, mode="nearest") if up2 else leaves[1][0]
        yr = F.leaky_relu(F.conv2d(xs, leaves[1][1], leaves[1][2], padding=1), slope)
        y = (DF.up2_conv3x3_act if up2 else DF.conv3x3_act)(*leaves[0], slope)
        assert bool((y[:, 0] == 0).all()) and bool((y[:, 1] < 0).all())
        y.backward(go)
        yr.backward(go)
        db, dbr = leaves[0][2].grad, leaves[1][2].grad
        want0, want1 = slope * float(go[:, 0].double().sum()), slope * float(go[:, 1].double().sum())
        tol0, tol1 = 1e-5 * float(go[:, 0].abs().sum()), 1e-5 * float(go[:, 1].abs().sum())   # fp32 sums of B * H * W terms
        assert abs(float(dbr[0]) - want0) <= tol0   # torch: the slope branch at exactly 0
        assert abs(float(db[0]) - want0) <= tol0 and abs(float(db[1]) - want1) <= tol1
        check(f"db up2={up2}", db, dbr, G_TOL)
        check(f"dw up2={up2}", leaves[0][1].grad, leaves[1][1].grad, G_TOL)
        check(f"dw of the zero / negative channels up2={up2}", leaves[0][1].grad[0:2], leaves[1][1].grad[0:2], G_TOL)
        check(f"dx up2={up2}", leaves[0][0].grad, leaves[1][0].grad, DX_TOL)
    # the 3conv chain: inner channel 0 of both activated maps exactly 0, channel 1 negative
    Cq = 4
    ps = [keyed_tensor("srzero3.w1", (Cq, C, 3, 3)), keyed_tensor("srzero3.b1", (Cq,)), keyed_tensor("srzero3.w2", (Cq, Cq, 1, 1)),
          keyed_tensor("srzero3.b2", (Cq,)), keyed_tensor("srzero3.w3", (C, Cq, 3, 3)), keyed_tensor("srzero3.b3", (C,))]
    ps = [p.to(dev) for p in ps]
    for wi, bi in ((0, 1), (2, 3)):
        ps[wi][0:2] = 0.0
        ps[bi][0], ps[bi][1] = 0.0, -0.25
    go = keyed_input("srzero3.go", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
    a = [t.clone().requires_grad_(True) for t in [x] + ps]
    r = [t.clone().requires_grad_(True) for t in [x] + ps]
    y = DF.conv3conv_res(a[0], *a[1:], x)
    yr = x + F.conv2d(F.leaky_relu(F.conv2d(F.leaky_relu(F.conv2d(r[0], r[1], r[2], padding=1), 0.2), r[3], r[4]), 0.2), r[5], r[6], padding=1)
    y.backward(go)
    yr.backward(go)
    check("3conv y", y, yr, Y_TOL)
    check("3conv dx", a[0].grad, r[0].grad, DX_TOL)
    for i in range(1, 7):
        check(f"3conv grad {i}", a[i].grad, r[i].grad, G_TOL)


# ---- bounds: one pass of every new entry point inside the red zones ------------------------------------------------------------------
def guarded(fn, *args):
    with redzone() as rz:
        fn(*args)
    assert rz.count > 0, "nothing was allocated through the patched helpers: the red zone checked nothing"


def test_red_zone_conv3x3_act(dev):
    guarded(_act_case, dev, 180, 64, 1, 13, 9, 0.01, False)
    guarded(_act_case, dev, 64, 180, 1, 13, 9, 0.2, False)


def test_red_zone_up2_conv3x3_act(dev):
    guarded(_act_case, dev, 64, 64, 1, 13, 9, 0.2, True)


def test_red_zone_conv3x3_ps_out(dev):
    guarded(_psout_case, dev, 60, 3, 3, 1, 13, 9)
    guarded(_psout_case, dev, 60, 3, 2, 1, 13, 9)


def test_red_zone_conv3conv_res(dev):
    guarded(_c3_case, dev, 48, 1, 13, 9)
    guarded(_c3_case, dev, 240, 1, 13, 9)


# ---- whole networks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upsampler,r,resi,embed,B,H,W", [("pixelshuffle", 8, "1conv", 36, 1, 8, 16), ("pixelshuffle", 3, "3conv", 48, 3, 16, 8),
                                                           ("pixelshuffledirect", 3, "3conv", 48, 3, 8, 24), ("nearest+conv", 2, "3conv", 48, 1, 24, 8)])
def test_net_vs_restatement(dev, upsampler, r, resi, embed, B, H, W):
    cfg = _cfg(upsampler, r, resi, embed)
    net = _net(cfg, dev, seed=r)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    x = keyed_input(f"srnet.x{r}", (B, 3, H, W)).to(dev)
    go = keyed_input(f"srnet.go{r}", (B, 3, r * H, r * W), lo=-1.0, hi=1.0).to(dev)
    xr, xg = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr = ref_sr_net(xr, P, cfg)
    yr.backward(go)
    y = net(xg)
    y.backward(go)
    check("y", y, yr, Y_TOL)
    check("dx", xg.grad, xr.grad, DX_TOL)
    for k, p in net.named_parameters():
        check("grad " + k, p.grad, P[k].grad, G_TOL)


@pytest.mark.parametrize("upsampler,r,resi,embed", [("pixelshuffle", 4, "1conv", 36), ("pixelshuffledirect", 3, "1conv", 36),
                                                    ("nearest+conv", 4, "3conv", 48)])
def test_batch_consistency_and_no_grad_bit_identity(dev, upsampler, r, resi, embed):
    net = _net(_cfg(upsampler, r, resi, embed), dev)
    x = keyed_input("srbatch", (3, 3, 16, 8)).to(dev)
    with torch.no_grad():
        yb = net(x)
        singles = torch.cat([net(x[i:i + 1]) for i in range(3)], 0)
    check("batched vs one image at a time", yb, singles, 1e-6)
    x.requires_grad_(True)
    yg = net(x)
    assert yg.requires_grad and torch.equal(yg.detach(), yb), "no_grad output must equal the grad-mode output bit for bit"


def test_backward_is_deterministic(dev):
    net = _net(_cfg("nearest+conv", 4, "3conv", 48), dev)
    x = keyed_input("srdet", (2, 3, 16, 8)).to(dev)
    grads = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        net(x).square().mean().backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_kernel_trace_counts(dev):
    from kernel_trace import kernel_trace

    net = _net(_cfg("nearest+conv", 4, "3conv", 48), dev)
    x = keyed_input("srtrace", (1, 3, 8, 8)).to(dev).requires_grad_(True)
    with kernel_trace() as tr:
        net(x).sum().backward()
        torch.cuda.synchronize()
    assert tr["swinsr_conv3conv_fwd"] == tr["swinsr_conv3conv_bwd"] == 7   # six RSTBs and conv_after_body
    assert tr["swinsr_conv_act_fwd"] == tr["swinsr_conv_act_bwd"] == 2     # conv_before_upsample, conv_hr
    assert tr["swinsr_up2_conv_act_fwd"] == tr["swinsr_up2_conv_act_bwd"] == 2
    net = _net(_cfg("pixelshuffledirect", 2), dev)
    with kernel_trace() as tr:
        net(x).sum().backward()
        torch.cuda.synchronize()
    assert tr["swinsr_ps_out_fwd"] == tr["swinsr_ps_out_bwd"] == 1


# ---- through SRModel at scale 4 ------------------------------------------------------------------------------------------------------------
def test_srmodel_training_step_vs_restatement(dev):
    """one SRModel.optimize_parameters at scale 4 (L1 + the fused AdamW) against the same step of the restatement with torch.optim.AdamW; the
    entries compared and the bound are those of test_gpu_rcan.py"""
    from basicsr.models import build_model

    lr = 1e-3
    cfg = _cfg("pixelshuffle", 4)
    opt = dict(name="t", model_type="SRModel", scale=4, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
               network_g=dict(type="SwinIR", **cfg), path=dict(),
               train=dict(pixel_opt=dict(type="L1Loss", loss_weight=1.0, reduction="mean"),
                          optim_g=dict(type="AdamW", lr=lr, weight_decay=0.01, fused=True)))
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    P0 = {k: v.detach().clone() for k, v in m.net_g.state_dict().items()}
    lq, gt = keyed_input("srstep.lq", (2, 3, 16, 16)), keyed_input("srstep.gt", (2, 3, 64, 64))
    m.feed_data({"lq": lq, "gt": gt})
    m.optimize_parameters(1)
    loss = float(m.log_dict["l_pix"])
    P = {k: v.clone().to(dev).requires_grad_(True) for k, v in P0.items()}
    ref_opt = torch.optim.AdamW(list(P.values()), lr=lr, weight_decay=0.01)
    lr_loss = F.l1_loss(ref_sr_net(lq.to(dev), P, cfg), gt.to(dev))
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
    """SRModel.test_tile at scale 4: each tile's interior equals the network run on that padded tile alone (tile 16 + pad 8: every padded
    tile is a multiple of the window)"""
    from basicsr.models import build_model

    size, pad, s = 16, 8, 4
    opt = dict(name="t", model_type="SRModel", scale=s, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="SwinIR", **_cfg("pixelshuffle", s)), path=dict(), tile=dict(infer_size=size, tile_pad=pad),
               val=dict(save_img=False))
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    img = keyed_input("srtile", (1, 3, 32, 48))
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
