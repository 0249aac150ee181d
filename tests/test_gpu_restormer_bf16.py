"""GPU: Restormer with bf16 activation storage (act_dtype="bf16", dcpt_amd/csrc/restormer_bf16.hip).

Accuracy yardstick of the bf16 blocks: the error of the HIP path against the float64 oracle must be within 1.5x (+ 4e-3) of the error of
a kernel-blind naive emulation (torch fp32 arithmetic, rounded to bf16 wherever the HIP path stores bf16: forward values AND the
gradients of those tensors); the networks against the goldens / the fp32 HIP net; save modes, batch consistency, repeatability bitwise."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import keyed_input, keyed_state_dict, keyed_tensor
from oracle import promptir_oracle as PR
from oracle import restormer_oracle as R

pytestmark = pytest.mark.gpu
R_CFG = dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, heads=[1, 2, 4, 8])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def relerr(a, b):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b, dtype=np.float64))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def frob(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).norm() / max(1e-12, float(b.norm())))


class _RoundBoth(torch.autograd.Function):
    """a bf16 store: the value is rounded, and so is the gradient that the backward pass stores for it"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().float()


rb = _RoundBoth.apply


def _ln(x, P, pre, eps):
    b, c, h, w = x.shape
    t = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
    sigma = t.var(-1, keepdim=True, unbiased=False)
    if pre + "body.bias" in P:
        t = (t - t.mean(-1, keepdim=True)) / torch.sqrt(sigma + eps) * P[pre + "body.weight"] + P[pre + "body.bias"]
    else:
        t = t / torch.sqrt(sigma + eps) * P[pre + "body.weight"]
    return t.reshape(b, h, w, c).permute(0, 3, 1, 2)


def naive_block(x, P, eps=1e-6, softmax=False):
    """one TransformerBlock in fp32 with bf16 rounding at the stored tensors (x itself enters rounded); eps / softmax: the PromptIR form"""
    b, c, h, w = x.shape
    heads = P["attn.temperature"].shape[0]
    x = rb(x)
    xn = rb(_ln(x, P, "norm1.", eps))
    qkv1 = rb(F.conv2d(xn, P["attn.qkv.weight"]))
    qkv = rb(F.conv2d(qkv1, P["attn.qkv_dwconv.weight"], padding=1, groups=3 * c))
    q, k, v = qkv.chunk(3, dim=1)
    q, k, v = (t.reshape(b, heads, c // heads, h * w) for t in (q, k, v))
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    pre = (q @ k.transpose(-2, -1)) * P["attn.temperature"]
    attn = pre.softmax(dim=-1) if softmax else F.relu(pre)
    out = rb((attn @ v).reshape(b, c, h, w))
    x = rb(x + F.conv2d(out, P["attn.project_out.weight"]))
    xn = rb(_ln(x, P, "norm2.", eps))
    u = rb(F.conv2d(xn, P["ffn.project_in.weight"]))
    a = F.conv2d(u, P["ffn.dwconv.weight"], padding=1, groups=u.shape[1])
    a1, a2 = a.chunk(2, dim=1)
    t = rb(F.gelu(a1) * a2)
    return rb(x + F.conv2d(t, P["ffn.project_out.weight"]))


def _block(lnt, dim, heads, variant="restormer"):
    """variant "promptir": the same block class with LayerNorm eps 1e-5 and softmax attention (DCPT_LN_EPS_1E5 | DCPT_ATTN_SOFTMAX)"""
    if variant == "promptir":
        from basicsr.archs.promptir_arch import TransformerBlock
    else:
        from basicsr.archs.restormer_arch import TransformerBlock

    blk = TransformerBlock(dim, heads, 2.66, False, lnt)
    blk.bf16 = True
    return blk


def _run_ref(fn, x, go, sd, dtype):
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.to(dtype).clone().requires_grad_(True)
    y = fn(xr, P)
    y.backward(go.to(dtype))
    return y.detach(), xr.grad, {k: p.grad for k, p in P.items()}


@pytest.mark.parametrize("dim,heads", [(48, 1), (96, 2), (192, 4), (384, 8)])
@pytest.mark.parametrize("lnt", ["BiasFree", "WithBias"])
@pytest.mark.parametrize("B,H,W", [(1, 13, 20), (3, 7, 9)])
@pytest.mark.parametrize("variant", ["restormer", "promptir"])
def test_block_error_vs_fp64_within_naive_bf16_emulation(dev, lnt, dim, heads, B, H, W, variant):
    blk = _block(lnt, dim, heads, variant)
    sd = {k: keyed_tensor(f"rb{lnt}{dim}." + k, tuple(v.shape)) for k, v in blk.state_dict().items()}
    sd["attn.temperature"] = sd["attn.temperature"].abs() + 0.5
    blk.load_state_dict(sd, strict=True)
    x = keyed_input(f"rb{dim}.x", (B, dim, H, W), lo=-1.0, hi=1.0).bfloat16().float()
    go = keyed_input(f"rb{dim}.go", (B, dim, H, W), lo=-1.0, hi=1.0).bfloat16().float()
    oracle = PR.transformer_block if variant == "promptir" else R.transformer_block
    y64, dx64, g64 = _run_ref(lambda t, P: oracle(t, P, ""), x, go, sd, torch.float64)
    naive = (lambda t, P: naive_block(t, P, 1e-5, True)) if variant == "promptir" else naive_block
    yn, dxn, gn = _run_ref(naive, x, go, sd, torch.float32)
    blk = blk.to(dev)
    xg = x.to(dev).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = blk(xg)
    assert y.dtype == torch.bfloat16
    y.backward(go.to(dev).bfloat16().contiguous(memory_format=torch.channels_last))
    pairs = [("y", y, yn, y64), ("dx", xg.grad, dxn, dx64)]
    pairs += [("grad " + k, p.grad, gn[k], g64[k]) for k, p in blk.named_parameters()]
    # The gradients that reach q and k run through F.normalize over the pixels, and at these sizes they are ill-conditioned in q and k
    # themselves: the one-ulp differences between two bf16 roundings of the depthwise output (HIP vs torch summation order) move the
    # gradients of dx, norm1, qkv and qkv_dwconv by up to 10-20 % (measured on MI355X), in the naive emulation and the HIP path alike,
    # either one the larger.  Those tensors are held to a Frobenius-norm bound that still catches a gross error (3x the naive error +
    # 0.05) and are checked tightly in test_mdta_bf16_backward_vs_exact_on_own_forward against exact math on the HIP path's own stored
    # q, k, v; the GDFN side and norm2 sit behind that noise too and get 1e-2 of absolute slack (measured worst: 1.7e-2 at 2.2e-2).
    qk_path = ("dx", "grad norm1.", "grad attn.qkv.", "grad attn.qkv_dwconv.")
    bad = []
    for name, mine, naive, ref in pairs:
        if name.startswith(qk_path):
            e_hip, e_naive = frob(mine.float(), ref), frob(naive, ref)
            if not (np.isfinite(e_hip) and e_hip <= 3.0 * e_naive + 0.05):
                bad.append(f"{name}: Frobenius err(HIP) {e_hip:.3e} > 3 * err(naive) {e_naive:.3e} + 0.05")
            continue
        e_hip, e_naive = relerr(mine.float(), ref), relerr(naive, ref)
        # (the temperature gradient is one scalar per head summed over ch x ch products of the normalised q, k: it carries the same noise,
        # as in the fp32 DCDist test; measured worst with softmax: 1.4e-2 against a 1.7e-2 bound)
        c = 4e-3 if name.startswith(("y", "grad attn.project_out")) else 1e-2
        if not (np.isfinite(e_hip) and e_hip <= 1.5 * e_naive + c):
            bad.append(f"{name}: err(HIP) {e_hip:.3e} > 1.5 * err(naive) {e_naive:.3e} + {c}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("C,heads,B,H,W", [(48, 1, 1, 13, 20), (96, 2, 1, 13, 20), (48, 1, 3, 7, 9), (48, 1, 1, 16, 16), (192, 4, 2, 9, 11)])
@pytest.mark.parametrize("save", ["full", "lean"])
@pytest.mark.parametrize("softmax", [False, True])
def test_mdta_bf16_backward_vs_exact_on_own_forward(dev, C, heads, B, H, W, save, softmax):
    """the whole MDTA backward against float64 math that starts from the q, k, v its forward stored (the ill-conditioned step from the
    depthwise output to q / k is then shared): dx (LayerNorm backward + residual), norm / qkv / depthwise / project_out / temperature
    gradients within bf16 storage error; softmax: the PromptIR form (softmax attention, LayerNorm eps 1e-5)"""
    from dcpt_amd import functional as DF

    g = lambda n, shp: keyed_tensor(f"own{C}.{n}", shp).to(dev).requires_grad_(True)
    nw, qw, dw, pw = g("nw", (C,)), g("qw", (3 * C, C, 1, 1)), g("dw", (3 * C, 1, 3, 3)), g("pw", (C, C, 1, 1))
    temp = (keyed_tensor(f"own{C}.t", (heads, 1, 1)).abs() + 0.5).to(dev).requires_grad_(True)
    x = keyed_input(f"own{C}.x", (B, C, H, W), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = keyed_input(f"own{C}.dy", (B, C, H, W), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    prev = DF.set_restormer_save(save)
    try:
        y = DF.mdta_bf16(x, nw, None, qw, dw, pw, temp, heads, True, eps_1e5=softmax, softmax=softmax)
    finally:
        DF.set_restormer_save(prev)
    qkv = y.grad_fn.saved_tensors[2]
    y.backward(dy)
    d = lambda t: t.detach().double().requires_grad_(True)
    leaf, tr, pwr = d(qkv), d(temp), d(pw)
    q, k, v = (t.reshape(B, heads, C // heads, H * W) for t in leaf.chunk(3, 1))
    pre = (F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)) * tr
    a = pre.softmax(dim=-1) if softmax else F.relu(pre)
    F.conv2d((a @ v).reshape(B, C, H, W), pwr).backward(dy.double())
    # below the stored q, k, v: LayerNorm (BiasFree) -> qkv 1x1 -> depthwise, driven by the reference gradient of q, k, v
    xr, nwr, qwr, dwr = d(x), d(nw), d(qw), d(dw)
    t = xr.permute(0, 2, 3, 1)
    xn = t / torch.sqrt(t.var(-1, keepdim=True, unbiased=False) + (1e-5 if softmax else 1e-6)) * nwr
    qkv_r = F.conv2d(F.conv2d(xn.permute(0, 3, 1, 2), qwr), dwr, padding=1, groups=3 * C)
    qkv_r.backward(leaf.grad)
    errs = {"temperature": relerr(temp.grad, tr.grad), "project_out": relerr(pw.grad, pwr.grad), "qkv_dwconv": relerr(dw.grad, dwr.grad),
            "qkv": relerr(qw.grad, qwr.grad), "norm": relerr(nw.grad, nwr.grad), "dx": relerr(x.grad.float(), xr.grad + dy.double())}
    bad = {k: e for k, e in errs.items() if not (np.isfinite(e) and e <= 2e-2)}
    assert not bad, f"scale-relative errors above 2e-2: {bad}"


def _net(name, dev, **kw):
    from basicsr.archs import build_network

    net = build_network(dict(type=name, **R_CFG, **kw))
    net.load_state_dict(keyed_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=0), strict=True)
    return net.to(dev)


def test_glue_bf16_vs_fp32(dev):
    """Down/Upsample convs, reduce_chan 1x1, pixel (un)shuffle, concat: the bf16 glue against the fp32 ops on the same (rounded) input"""
    from dcpt_amd import functional as DF

    x = keyed_input("glue.x", (2, 32, 12, 10), lo=-1, hi=1).bfloat16().float().to(dev).contiguous(memory_format=torch.channels_last)
    s = keyed_input("glue.s", (2, 16, 24, 20), lo=-1, hi=1).bfloat16().float().to(dev).contiguous(memory_format=torch.channels_last)
    w3 = keyed_tensor("glue.w3", (32, 32, 3, 3)).to(dev)
    w1 = keyed_tensor("glue.w1", (8, 32, 1, 1)).to(dev)
    outs = {}
    for dt in (torch.float32, torch.bfloat16):
        xa = x.detach().to(dt).clone(memory_format=torch.channels_last).requires_grad_(True)
        sa = s.detach().to(dt).clone(memory_format=torch.channels_last).requires_grad_(True)
        wa, wb = w3.clone().requires_grad_(True), w1.clone().requires_grad_(True)
        up = DF.pixel_shuffle2(DF.conv_nobias(xa, wa))                       # Upsample: [2, 8, 24, 20]
        cat = DF.concat_channels(up, sa)                                     # [2, 24, 24, 20] -> unshuffle to 96 ch
        dn = DF.pixel_unshuffle2(cat)
        y = DF.conv_nobias(dn[:, :32].contiguous(memory_format=torch.channels_last), wb)
        gy = keyed_input("glue.gy", tuple(y.shape), lo=-1, hi=1).to(dev).to(dt).contiguous(memory_format=torch.channels_last)
        y.backward(gy)
        outs[dt] = (y.float(), xa.grad.float(), sa.grad.float(), wa.grad, wb.grad)
    for name, a, b in zip(("y", "dx", "dskip", "dw3", "dw1"), outs[torch.bfloat16], outs[torch.float32]):
        e = relerr(a, b)
        assert e <= 2e-2, f"{name}: {e:.3e}"


# The network-level bounds were measured on MI355X (this file's first runs): the bf16 forward stays within a few per cent of the fp32
# result (tiny nets 1-2.5e-2, the default net at B = 2, 128 x 128 7.3e-2 scale-relative -- above the 3e-2 of the NAFNet bf16 suite:
# 36 transformer blocks of rounding, each with the normalised attention); the gradients of everything below the first q / k rounding
# carry the ill-conditioning described in test_block_error_vs_fp64_within_naive_bf16_emulation (tiny nets: 2e-2 .. 3e-1 max-relative
# per tensor), so they are checked by direction (cosine) rather than by max error.
def _cos(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)).flatten()
    b = torch.as_tensor(np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)).flatten()
    return float(F.cosine_similarity(a, b, dim=0))


@pytest.mark.parametrize("tag,name", [("restormer", "Restormer"), ("restormer_origin", "Restormer_origin")])
def test_restormer_tiny_golden_bf16(dev, golden_dir, tag, name):
    g = np.load(os.path.join(golden_dir, f"{tag}_tiny.npz"))
    net = _net(name, dev, act_dtype="bf16")
    x = keyed_input(f"{tag}.x", (2, 3, 32, 32)).to(dev).requires_grad_(True)
    gw = keyed_input(f"{tag}.gw", (2, 3, 32, 32), lo=-1.0, hi=1.0).to(dev)
    taps = []
    if name == "Restormer":
        for n, m in net.named_modules():
            if "decoder_level" in n and n.count(".") == 1:
                m.register_forward_hook(lambda mod, i, o: taps.append(o))
    y = net(x)
    assert y.dtype == torch.float32
    (y * gw).sum().backward()
    e = relerr(y, g["y"])
    assert e <= 3e-2, f"y: {e:.3e}"
    params = dict(net.named_parameters())
    coss = {"dx": _cos(x.grad, g["dx"])}
    for k in g.files:
        if k.startswith("g.") and k != "g_names":
            coss[k[2:]] = _cos(params[k[2:]].grad, g[k])
    bad = {k: c for k, c in coss.items() if not (np.isfinite(c) and c >= 0.95)}
    assert not bad, f"gradient cosine below 0.95: {bad}"
    if name == "Restormer":
        assert [t.dtype for t in taps] == [torch.bfloat16] * 3


def test_default_net_bf16_vs_fp32(dev):
    from basicsr.archs import build_network

    out, grads = {}, {}
    x = keyed_input("rdef.x", (2, 3, 128, 128)).to(dev)
    gw = keyed_input("rdef.gw", (2, 3, 128, 128), lo=-1.0, hi=1.0).to(dev)
    for dt in ("fp32", "bf16"):
        net = build_network(dict(type="Restormer", act_dtype=dt))
        net.load_state_dict(keyed_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=3), strict=True)
        net = net.to(dev)
        y = net(x)
        (y * gw).sum().backward()
        out[dt] = y.detach()
        grads[dt] = {k: p.grad.detach().double().flatten() for k, p in net.named_parameters()}
        del net
    e = relerr(out["bf16"], out["fp32"])
    assert e <= 1e-1, f"output: scale-relative error {e:.3e} > 1e-1"
    # Measured at B = 2 (MI355X): output 7.3e-2 scale-relative; per-tensor gradient cosines 0.84 .. 1.0 -- the q / k path (norm1, qkv,
    # qkv_dwconv) down to 0.845, other tensors of the wide levels down to 0.869 (they see the q / k noise of the blocks after them
    # through dx).  The 0.99 of the NAFNet bf16 suite does not hold for this network; the bound is 0.8 for every tensor.
    coss = {k: float(F.cosine_similarity(grads["bf16"][k], grads["fp32"][k], dim=0)) for k in grads["fp32"] if float(grads["fp32"][k].norm()) > 0}
    bad = {k: round(c, 4) for k, c in coss.items() if not c >= 0.8}
    assert not bad, f"gradient cosines below bound: {bad}"


def _step(net, x, gw):
    net.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y = net(xg)
    (y * gw).sum().backward()
    return y.detach().clone(), xg.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters()}


def _same(a, b):
    ya, dxa, ga = a
    yb, dxb, gb = b
    assert torch.equal(ya, yb) and torch.equal(dxa, dxb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("name", ["Restormer", "Restormer_origin"])
def test_save_modes_bit_identical_bf16(dev, name):
    x = keyed_input("rsm.x", (2, 3, 32, 24)).to(dev)
    gw = keyed_input("rsm.gw", (2, 3, 32, 24), lo=-1.0, hi=1.0).to(dev)
    res = {}
    for mode in ("full", "balanced", "lean"):
        net = _net(name, dev, act_dtype="bf16", save_mode=mode)
        res[mode] = _step(net, x, gw)
    _same(res["full"], res["balanced"])
    _same(res["full"], res["lean"])


def test_batch_consistency_and_repeatability_bf16(dev):
    net = _net("Restormer", dev, act_dtype="bf16")
    x = keyed_input("rbc.x", (3, 3, 24, 40)).to(dev)
    gw = keyed_input("rbc.gw", (3, 3, 24, 40), lo=-1.0, hi=1.0).to(dev)
    a, b = _step(net, x, gw), _step(net, x, gw)
    _same(a, b)
    for i in range(3):
        one = _step(net, x[i:i + 1], gw[i:i + 1])
        assert torch.equal(one[0], a[0][i:i + 1]), f"sample {i}: output differs from its batch"
        assert torch.equal(one[1], a[1][i:i + 1]), f"sample {i}: input gradient differs from its batch"


def test_no_grad_keeps_nothing_bf16(dev):
    net = _net("Restormer", dev, act_dtype="bf16")
    x = keyed_input("rng.x", (1, 3, 16, 16)).to(dev)
    packed = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(1) or t, lambda t: t):
        with torch.no_grad():
            y = net(x)
        assert not packed and y.grad_fn is None
        y2 = net(x)
    assert packed and torch.equal(y, y2.detach())


def test_launch_trace_bf16_step(dev):
    from dcpt_amd import _lib

    lib = _lib.load()
    net = _net("Restormer", dev, act_dtype="bf16", save_mode="balanced")
    x = keyed_input("rtr.x", (1, 3, 16, 16)).to(dev)
    _step(net, x, torch.ones_like(x))   # warm-up outside the trace
    torch.cuda.synchronize()
    lib.dcpt_trace_enable(1)
    try:
        _step(net, x, torch.ones_like(x))
        torch.cuda.synchronize()
        n = lib.dcpt_trace_read(None, 0)
        import ctypes

        buf = ctypes.create_string_buffer(n)
        lib.dcpt_trace_read(buf, n)
    finally:
        lib.dcpt_trace_enable(0)
    counts = {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines() if ln.strip()}
    nb = 8   # transformer blocks of R_CFG: 3 encoder + latent + 3 decoder + 1 refinement
    # per block, balanced mode: LayerNorm 2 forward + 2 recomputed in backward; Gram: forward + dattn; apply: attn v, its recomputation,
    # dv, dq, dk; the GDFN gate forward + its recomputation; one backward of each depthwise form
    expect = {"rst_bf16.ln_fwd": 4, "rst_bf16.ln_bwd": 2, "rst_bf16.dw_sq_fwd": 1, "rst_bf16.gram": 2, "rst_bf16.apply": 5,
              "dw.ring_gelu_fwd_bf16": 2, "dw.ring_bwd_gelu_bf16": 1, "rst_bf16.dw_plain_bwd": 1}
    for tag, per in expect.items():
        assert counts.get(tag, 0) == per * nb, (tag, counts.get(tag, 0), per * nb, counts)
    # glue: 3 downsamples + 3 upsamples (pixel (un)shuffle forward + backward), 3 concats (+ splits in backward)
    assert counts.get("rst_bf16.pixel_shuffle", 0) == 12 and counts.get("rst_bf16.concat", 0) == 6, counts
    # no fp32 Restormer kernel ran
    assert not any(k.startswith(("dw.ring_fwd_f32", "dw.ring_bwd_f32", "dw.reg_fwd_f32", "dw.reg_bwd_f32")) for k in counts), counts
