"""GPU: RCAN inference on bf16 activation storage (``RCAN(act_dtype="bf16")`` over dcpt_rcab_fwd_bf16, dcpt_conv3x3_res_fwd_bf16,
dcpt_conv3x3_ps_fwd_bf16).

Accuracy yardstick (the project's own for bf16 storage, tests/test_gpu_bf16.py): for a tensor with float64 truth T,
    err(HIP) <= 1.5 * err(naive) + 4e-3,      err = max|. - T| / max|T|
4e-3 is one bf16 ulp at the tensor's scale, 1.5 covers the spread of a max-norm.  ``naive`` is a kernel-blind torch emulation (below): the
RCAB / network arithmetic restated in fp32 on the CPU, rounded to torch.bfloat16 at exactly the storage points of the bf16 path -- block
input, the conv weight operand copies, h, t, y, the group-conv / conv_after_body / upsample outputs -- with fp32 biases, accumulation,
pooled mean (of t before its rounding), CA FCs and sigmoid.  T is the same restatement in float64 without any rounding, or the golden
vector of the real reference where tests/golden holds one.

The new epilogues exist on the 128-row GEMM kernel only (gemm_nt_bf16_256_ok / _tall_ok refuse them), so there is no other tile class to
reach: every case asserts that the trace names ``nt_bf16.128_conv3``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor

pytestmark = pytest.mark.gpu
TINY = dict(num_in_ch=3, num_out_ch=3, num_feat=32, num_group=2, num_block=2)
TINY_LR = (2, 3, 11, 13)
MEAN = (0.4488, 0.4371, 0.4040)
BF = torch.bfloat16


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


# ---- the restatement: rnd = bf16 rounding at the storage points in fp32 (naive), or the identity in float64 (truth); CPU ------------------
def rnd_bf16(t):
    return t.to(BF).to(t.dtype)


def ident(t):
    return t


def re_rcab(x, P, pre, res_scale, rnd):
    """x: the block input as stored (already rnd'ed)"""
    h = rnd(F.relu(F.conv2d(x, rnd(P[pre + "rcab.0.weight"]), P[pre + "rcab.0.bias"], padding=1)))
    tf = F.conv2d(h, rnd(P[pre + "rcab.2.weight"]), P[pre + "rcab.2.bias"], padding=1)
    a = tf.mean((2, 3), keepdim=True)   # of the values before their rounding
    a = F.relu(F.conv2d(a, P[pre + "rcab.3.attention.1.weight"], P[pre + "rcab.3.attention.1.bias"]))
    a = torch.sigmoid(F.conv2d(a, P[pre + "rcab.3.attention.3.weight"], P[pre + "rcab.3.attention.3.bias"]))
    return rnd(x + res_scale * (rnd(tf) * a))


def re_net(x, P, cfg, upscale, rnd, res_scale=1.0, img_range=255.0):
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    xf = rnd(F.conv2d((x - mean) * img_range, P["conv_first.weight"], P["conv_first.bias"], padding=1))
    t = xf
    for gi in range(cfg.get("num_group", 10)):
        t0 = t
        for b in range(cfg.get("num_block", 16)):
            t = re_rcab(t, P, f"body.{gi}.residual_group.{b}.", res_scale, rnd)
        t = rnd(F.conv2d(t, rnd(P[f"body.{gi}.conv.weight"]), P[f"body.{gi}.conv.bias"], padding=1) + t0)
    t = rnd(F.conv2d(t, rnd(P["conv_after_body.weight"]), P["conv_after_body.bias"], padding=1) + xf)
    stages = [2] * (upscale.bit_length() - 1) if upscale & (upscale - 1) == 0 else [3]
    for i, r in enumerate(stages):
        t = rnd(F.pixel_shuffle(F.conv2d(t, rnd(P[f"upsample.{2 * i}.weight"]), P[f"upsample.{2 * i}.bias"], padding=1), r))
    return F.conv2d(t, P["conv_last.weight"], P["conv_last.bias"], padding=1) / img_range + mean


def naive_and_truth(fn, x, P, *a, **k):
    """(naive fp32 with bf16 storage points, float64 truth) of a restatement on the CPU"""
    with torch.no_grad():
        naive = fn(x.float(), {n: v.float() for n, v in P.items()}, *a, rnd=rnd_bf16, **k)
        truth = fn(x.double(), {n: v.double() for n, v in P.items()}, *a, rnd=ident, **k)
    return naive, truth


def _cpu_sd(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def _net(cfg, dev, seed=0, act_dtype="bf16"):
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


def _bf16_map(x, dev):
    """a CPU fp32 NCHW tensor as the bf16 channels_last device map the kernels take"""
    return x.to(dev).to(BF).contiguous(memory_format=torch.channels_last)


# ---- 1. RCAB against the truth ------------------------------------------------------------------------------------------------------
# golden blocks (tools/make_golden_rcan.py): M = 442 -- ragged last tiles, and the second image begins inside a 128-row block of the batch
# (conv1's tile straddles the two images; conv2's per-image tiles fill one more column-sum row than the image has tiles); N = 32 is below
# one 64-column tile; the third has res_scale = 0.5
GOLDEN_BLOCKS = [("c64_s16", 64, 16, 1.0, 2, 13, 17), ("c32_s4", 32, 4, 1.0, 2, 13, 17), ("c64_s16_rs05", 64, 16, 0.5, 2, 13, 17)]
# the 128-column class with more than two images inside one 128-row tile; Cr = 1 with K = 72 (a ragged last k-tile); several tiles per image
OTHER_BLOCKS = [(128, 16, 3, 5, 6), (8, 8, 4, 7, 9), (64, 16, 5, 31, 29)]


def _run_block(blk, x, dev):
    from kernel_trace import kernel_trace

    with torch.no_grad(), kernel_trace() as tr:
        y = blk(_bf16_map(x, dev))
        torch.cuda.synchronize()
    assert y.dtype == BF and y.shape == x.shape
    tr.assert_ran("rcan_bf16.rcab_fwd", "nt_bf16.128_conv3")
    tr.assert_not_ran("rcan_rcab_fwd", "nt_bf16.256_conv3", "nt_bf16.tall512_conv3")
    assert tr["rcan_bf16.rcab_fwd"] == 1 and tr["nt_bf16.128_conv3"] == 2
    return y


@pytest.mark.parametrize("tag,C_,sq,rs,B,H,W", GOLDEN_BLOCKS)
def test_rcab_vs_golden(dev, golden_dir, tag, C_, sq, rs, B, H, W):
    g = np.load(os.path.join(golden_dir, f"rcan_block_{tag}.npz"))
    blk = _rcab(C_, sq, rs, dev, tag=tag)
    x = keyed_input(f"rcab_{tag}.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    y = _run_block(blk, x, dev)
    naive, truth = naive_and_truth(lambda x_, P, rnd: re_rcab(rnd(x_), P, "", rs, rnd), x, _cpu_sd(blk))
    assert err(truth, g["y"]) < 1e-5   # the float64 restatement is the reference's arithmetic
    yardstick(f"rcab {tag}", y, naive, g["y"])


@pytest.mark.parametrize("C_,sq,B,H,W", OTHER_BLOCKS)
def test_rcab_vs_float64(dev, C_, sq, B, H, W):
    blk = _rcab(C_, sq, 0.5, dev, seed=C_)
    x = keyed_input(f"rcanb{C_}", (B, C_, H, W), lo=-1.0, hi=1.0)
    y = _run_block(blk, x, dev)
    naive, truth = naive_and_truth(lambda x_, P, rnd: re_rcab(rnd(x_), P, "", 0.5, rnd), x, _cpu_sd(blk))
    yardstick(f"rcab C={C_}", y, naive, truth)


# ---- 2. the upsample stage and the residual conv alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,C_,B,H,W", [(2, 32, 3, 9, 7), (3, 64, 1, 16, 24)])
def test_upsample_stage_vs_float64(dev, r, C_, B, H, W):
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    w = keyed_tensor(f"psb{r}.weight", (r * r * C_, C_, 3, 3))
    b = keyed_tensor(f"psb{r}.bias", (r * r * C_,))
    x = keyed_input(f"psb{r}.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    with torch.no_grad(), kernel_trace() as tr:
        y = DF.conv3x3_ps_bf16(_bf16_map(x, dev), w.to(dev), b.to(dev), r)
        torch.cuda.synchronize()
    assert y.dtype == BF and tuple(y.shape) == (B, C_, r * H, r * W)
    tr.assert_ran("rcan_bf16.ps_fwd", "nt_bf16.128_conv3")
    tr.assert_not_ran("rcan_ps_fwd")

    def stage(x_, P, rnd):
        return rnd(F.pixel_shuffle(F.conv2d(rnd(x_), rnd(P["w"]), P["b"], padding=1), r))

    naive, truth = naive_and_truth(stage, x, {"w": w, "b": b})
    yardstick(f"upsample r={r}", y, naive, truth)


def test_residual_conv_vs_float64(dev):
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    C_, B, H, W = 64, 2, 13, 17
    w, b = keyed_tensor("resb.weight", (C_, C_, 3, 3)), keyed_tensor("resb.bias", (C_,))
    x = keyed_input("resb.x", (B, C_, H, W), lo=-1.0, hi=1.0)
    res = keyed_input("resb.res", (B, C_, H, W), lo=-1.0, hi=1.0)
    with torch.no_grad():
        scale = float(F.conv2d(x, w, b, padding=1).abs().max())
    res = res * (8.0 * scale)   # a residual of another magnitude than the conv output
    with torch.no_grad(), kernel_trace() as tr:
        y = DF.conv3x3_res_bf16(_bf16_map(x, dev), w.to(dev), b.to(dev), _bf16_map(res, dev))
        torch.cuda.synchronize()
    tr.assert_ran("rcan_bf16.res_fwd", "nt_bf16.128_conv3")

    def conv(x_, P, rnd):
        return rnd(F.conv2d(rnd(x_), rnd(P["w"]), P["b"], padding=1) + rnd(P["res"]))

    naive, truth = naive_and_truth(conv, x, {"w": w, "b": b, "res": res})
    yardstick("residual conv", y, naive, truth)
    # the conv itself must be right too, not only the (larger) residual: the same bound on y - res at the conv output's scale
    r16 = res.to(BF).double()
    yardstick("residual conv, conv part", y.detach().cpu().double() - r16, naive.double() - r16, truth - r16)


# ---- 3. tiny nets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_tiny_net_golden(dev, golden_dir, s):
    from kernel_trace import kernel_trace

    g = np.load(os.path.join(golden_dir, f"rcan_tiny_x{s}.npz"))
    cfg = dict(TINY, upscale=s)
    net = _net(cfg, dev)
    x = keyed_input(f"rcant{s}.x", TINY_LR)
    with torch.no_grad(), kernel_trace() as tr:
        y = net(x.to(dev))
        torch.cuda.synchronize()
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(g["y"].shape)
    assert tr["rcan_rcab_fwd"] == 0 and tr["rcan_ps_fwd"] == 0, tr.counts
    assert tr["rcan_bf16.rcab_fwd"] == TINY["num_group"] * TINY["num_block"]
    assert tr["rcan_bf16.res_fwd"] == TINY["num_group"] + 1 and tr["rcan_bf16.ps_fwd"] == (2 if s == 4 else 1)
    tr.assert_not_ran("rcan_bf16.wpack_per_call")
    naive, truth = naive_and_truth(re_net, x, _cpu_sd(net), cfg, s)
    assert err(truth, g["y"]) < 1e-5
    yardstick(f"tiny x{s}", y, naive, g["y"])
    net.set_act_dtype("fp32")   # the same network object back on today's path
    with kernel_trace() as tr:
        y32 = net(x.to(dev).requires_grad_(True))
        torch.cuda.synchronize()
    assert tr["rcan_rcab_fwd"] == 4 and tr["rcan_bf16.rcab_fwd"] == 0 and y32.requires_grad
    e = err(y32, g["y"])
    assert e <= 5e-5, f"fp32 after the switch: {e:.3e}"


# ---- 4. the default net --------------------------------------------------------------------------------------------------------------------
def test_default_net_golden(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "rcan_full.npz"))
    cfg = dict(num_in_ch=3, num_out_ch=3)
    net = _net(cfg, dev)
    with torch.no_grad():   # tools/make_golden_rcan.py damp_, as tests/test_gpu_rcan.py::test_default_net_golden
        for k, p in net.named_parameters():
            if ".rcab.2." in k:
                p.mul_(0.1)
    assert list(net.state_dict().keys()) == list(g["keys"]) and len(net.state_dict()) == 1310
    x = keyed_input("rcanf.x", (1, 3, 12, 12))
    with torch.no_grad():
        y = net(x.to(dev))
    naive, truth = naive_and_truth(re_net, x, _cpu_sd(net), cfg, 4)
    assert err(truth[..., ::4, ::4], g["y_sub"]) < 1e-5
    yardstick("default net", y[..., ::4, ::4], naive[..., ::4, ::4], g["y_sub"])


# ---- 5. determinism, batch consistency -------------------------------------------------------------------------------------------------------
def test_determinism_and_batch_consistency(dev):
    cfg = dict(TINY, upscale=3)
    net = _net(cfg, dev)
    x = keyed_input("rcanbatch", (3, 3, 13, 10))
    with torch.no_grad():
        yb = net(x.to(dev))
        assert torch.equal(net(x.to(dev)), yb), "two runs must agree bit for bit"
        singles = torch.cat([net(x[i:i + 1].to(dev)) for i in range(3)], 0)
    naive, truth = naive_and_truth(re_net, x, _cpu_sd(net), cfg, 3)
    yardstick("batched", yb, naive, truth)
    # two bf16 evaluations: apart by no more than the yardstick's right-hand side
    d, bound = err(yb.double().cpu() - singles.double().cpu() + truth, truth), 1.5 * err(naive, truth) + 4e-3
    print(f"batched vs one at a time: {d:.3e} (bound {bound:.3e})")
    assert d <= bound
    # and in fact equal: the conv2 GEMM of an RCAB tiles its rows per image, so the pooled sums are not split by the batch (EB_BIASCOL)
    assert torch.equal(yb, singles)


# ---- 6. inference only, nothing kept -------------------------------------------------------------------------------------------------------
def test_inference_only_and_memory(dev):
    net = _net(dict(TINY, upscale=4), dev)
    x = keyed_input("rcanmem", (2, 3, 32, 32)).to(dev)
    with pytest.raises(NotImplementedError, match="inference-only"):
        net(x)
    with pytest.raises(NotImplementedError, match="inference-only"):
        net.requires_grad_(False)
        try:
            net(x.clone().requires_grad_(True))
        finally:
            net.requires_grad_(True)

    def peak(act_dtype):
        net.set_act_dtype(act_dtype)
        with torch.no_grad():
            net(x)   # workspaces (and weight packs) grown
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
    print(f"peak above the resident state: bf16 {p16} B, fp32 {p32} B")
    assert p16 < p32


# ---- 7. exact-size workspaces under red zones -----------------------------------------------------------------------------------------------
def test_exact_workspaces_and_short_workspace_refused(dev):
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace
    from redzone import redzone

    lib = _lib.load()
    C_, sq, B, H, W = 64, 16, 2, 13, 17
    blk = _rcab(C_, sq, 1.0, dev, seed=7)
    x = _bf16_map(keyed_input("rcanrz.x", (B, C_, H, W), lo=-1.0, hi=1.0), dev)
    w2, b2 = keyed_tensor("rcanrz.w2", (4 * C_, C_, 3, 3)).to(dev), keyed_tensor("rcanrz.b2", (4 * C_,)).to(dev)
    w3, b3 = keyed_tensor("rcanrz.w3", (9 * C_, C_, 3, 3)).to(dev), keyed_tensor("rcanrz.b3", (9 * C_,)).to(dev)
    c1 = blk.rcab[0]
    with torch.no_grad():
        ref = [blk(x), DF.conv3x3_res_bf16(x, c1.weight, c1.bias, x), DF.conv3x3_ps_bf16(x, w2, b2, 2), DF.conv3x3_ps_bf16(x, w3, b3, 3)]
        with redzone() as rz:
            got = [blk(x), DF.conv3x3_res_bf16(x, c1.weight, c1.bias, x), DF.conv3x3_ps_bf16(x, w2, b2, 2), DF.conv3x3_ps_bf16(x, w3, b3, 3)]
        assert rz.count >= 8
    for a, b in zip(ref, got):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    # one byte short: refused before any launch
    ps = [t.detach() for t in (c1.weight, c1.bias, blk.rcab[2].weight, blk.rcab[2].bias, blk.rcab[3].attention[1].weight,
                               blk.rcab[3].attention[1].bias, blk.rcab[3].attention[3].weight, blk.rcab[3].attention[3].bias)]
    pp = _lib.RcabParams(*[t.data_ptr() for t in ps])
    y = torch.empty_like(x)
    y4 = torch.empty((B, 9 * H, W, C_), dtype=BF, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    need = [lib.dcpt_rcab_bf16_ws_bytes(B, H, W, C_, C_ // sq), lib.dcpt_conv3x3_res_bf16_ws_bytes(B, H, W, C_),
            lib.dcpt_conv3x3_ps_bf16_ws_bytes(B, H, W, C_, 3)]
    ws = torch.empty(max(need), dtype=torch.uint8, device=dev)
    with kernel_trace() as tr:
        rcs = [lib.dcpt_rcab_fwd_bf16(C.byref(pp), None, 0, None, 0, x.data_ptr(), y.data_ptr(), ws.data_ptr(), need[0] - 1, B, H, W, C_, C_ // sq,
                                      1.0, st),
               lib.dcpt_conv3x3_res_fwd_bf16(x.data_ptr(), ps[0].data_ptr(), None, 0, ps[1].data_ptr(), x.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                             need[1] - 1, B, H, W, C_, st),
               lib.dcpt_conv3x3_ps_fwd_bf16(x.data_ptr(), w3.data_ptr(), None, 0, b3.data_ptr(), y4.data_ptr(), ws.data_ptr(), need[2] - 1, B, H, W,
                                            C_, 3, st)]
    assert all(rc != 0 for rc in rcs), rcs
    assert "workspace too small" in lib.dcpt_last_error().decode()
    assert tr.counts == {}, f"a refused call launched: {tr.counts}"


# ---- 8. weight packs ------------------------------------------------------------------------------------------------------------------------
def test_weight_packs(dev, monkeypatch):
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    net = _net(dict(TINY, upscale=2), dev)
    nconv = TINY["num_group"] * (2 * TINY["num_block"] + 1) + 1 + 1
    x = keyed_input("rcanpack", (2, 3, 11, 13)).to(dev)
    with torch.no_grad():
        y = net(x)
        assert DF.pack_convs_bf16(net._convs_bf16()) == 0 and len(net._convs_bf16()) == nconv   # packed once, current
        with kernel_trace() as tr:
            assert torch.equal(net(x), y)
        tr.assert_not_ran("rcan_bf16.wpack_per_call", "head.wpack_multi")
        # the per-call-pack forward (wpacked = NULL at every entry point) is bit-identical
        monkeypatch.setattr(DF, "CONV_PACK_CACHE", False)
        with kernel_trace() as tr:
            y_call = net(x)
        assert tr["rcan_bf16.wpack_per_call"] == nconv
        monkeypatch.setattr(DF, "CONV_PACK_CACHE", True)
        assert torch.equal(y_call, y)
        # an in-place edit makes exactly that pack stale
        net.body[1].residual_group[0].rcab[2].weight.mul_(1.5)
        assert DF.pack_convs_bf16(net._convs_bf16()) == 1
        y_edit = net(x)
        assert not torch.equal(y_edit, y)
        monkeypatch.setattr(DF, "CONV_PACK_CACHE", False)
        assert torch.equal(net(x), y_edit)
        monkeypatch.setattr(DF, "CONV_PACK_CACHE", True)
        # load_state_dict makes every pack stale
        sd = {k: (v * 0.5 if k.endswith("conv_after_body.weight") else v.clone()) for k, v in net.state_dict().items()}
        net.load_state_dict(sd, strict=True)
        assert DF.pack_convs_bf16(net._convs_bf16()) == nconv
        y_load = net(x)
        assert not torch.equal(y_load, y_edit)
        monkeypatch.setattr(DF, "CONV_PACK_CACHE", False)
        assert torch.equal(net(x), y_load)


# ---- 9. SRModel ------------------------------------------------------------------------------------------------------------------------------
def _srmodel(act_dtype, **extra):
    from basicsr.models import build_model

    opt = dict(name="t", model_type="SRModel", scale=4, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="RCAN", act_dtype=act_dtype, **dict(TINY, upscale=4)), path=dict(), val=dict(save_img=False), **extra)
    m = build_model(opt)
    fill_module_(m.net_g, seed=0)
    return m


def _tiles_alone(m, img, dev, size=16, pad=4, s=4):
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
    return want


def test_srmodel_tiled_inference_equals_tiles_alone(dev):
    """SRModel.test_tile with network_g.act_dtype: bf16 at scale 4: each tile's interior equals the bf16 network run on that padded tile alone,
    bit for bit.  test_tile stacks tiles of equal padded shape into one batch (here 4 corner and 2 edge tiles) and runs the batches on two
    streams, so this also pins that a batched bf16 forward is the one-image forwards: per-image row tiles in the column-sum GEMM."""
    m = _srmodel("bf16", tile=dict(infer_size=16, tile_pad=4))
    assert m.net_g.act_dtype == "bf16"
    img = keyed_input("rcantile", (1, 3, 32, 48))
    m.feed_data({"lq": img})
    m.pre_test()
    m.test_tile()
    m.post_test()
    got = m.output.cpu()
    assert tuple(got.shape) == (1, 3, 128, 192)
    want = _tiles_alone(m, img, dev)
    nbad = int((got != want).sum())
    print(f"tiled vs tiles alone: {nbad} of {got.numel()} elements differ, max {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want)


def test_srmodel_selfensemble_vs_fp32(dev):
    img = keyed_input("rcanens", (1, 3, 32, 48))
    outs = {}
    for act in ("fp32", "bf16"):
        m = _srmodel(act)
        m.feed_data({"lq": img})
        m.test_selfensemble()
        outs[act] = m.output.cpu()
        sd = _cpu_sd(m.net_g)
    # the naive emulation of the same x8 ensemble (the dihedral group as flips / transpose of the input, undone on the output)
    cfg = dict(TINY, upscale=4)
    acc = 0
    for k in range(8):
        fwd = (lambda t: t.transpose(-1, -2)) if k & 4 else ident
        a = fwd(img)
        a = a.flip(-2) if k & 2 else a
        a = a.flip(-1) if k & 1 else a
        with torch.no_grad():
            o = re_net(a.contiguous(), sd, cfg, 4, rnd_bf16)
        o = o.flip(-1) if k & 1 else o
        o = o.flip(-2) if k & 2 else o
        acc = acc + fwd(o)
    yardstick("self-ensemble vs the fp32 ensemble", outs["bf16"], acc / 8, outs["fp32"])
