"""GPU: the token-tap classifier head (PromptIR_NoImg_DC(downsample=True), reference degrad_classify_arch.py:622-641) and the SwinIR
DCPT step around it -- the strided mixing kernels against a float64 restatement, the in-place merge of the strided tap's gradient, the
head and the step against golden vectors of the real reference, the other model paths and the command line."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = 29   # tools/make_golden_swinir.py: gradients above 4096 elements are stored as every 29th element
SWIN_TINY = dict(img_size=16, embed_dim=36, depths=[2] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
STEP_HEAD = dict(feature_dims=[36, 36, 36], num_res_blocks=1, num_classes=5, downsample=True)
# (B, C, H, W, s): one float4 group per pixel; SwinIR's width (45 groups, not a power of two) over more than one block of the backward;
# a coarse map of height 1; s == 1
SHAPES = [(1, 4, 4, 8, 2), (2, 180, 8, 8, 4), (3, 12, 4, 8, 4), (2, 36, 16, 16, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def check(name, a, b, tol):
    e = relerr(a, b)
    print(f"{name}: scale-relative max error {e:.3e} (bound {tol:.1e})")
    assert np.isfinite(e) and e <= tol, f"{name}: scale-relative max error {e:.3e} > {tol:.1e}"


def _nhwc(t):
    n, c, h, w = t.shape
    out = torch.empty_strided((n, c, h, w), (h * w * c, 1, w * c, c), dtype=t.dtype, device=t.device)
    return out.copy_(t)


# ---- kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "batch_slice", "grid_view"])
@pytest.mark.parametrize("use_prev", [True, False])
@pytest.mark.parametrize("B,C,H,W,s", SHAPES)
def test_strided_mix_vs_float64(dev, B, C, H, W, s, use_prev, form):
    """prev + softmax(mw)[i] * feat[:, :, ::s, ::s] and its autograd in float64 against dcpt_mix_stride_* (per-op bound of DESIGN.md
    section 2: 1e-5 scale-relative).  batch_slice: rows 2..3 of a batch of 4 (the batch stride is not the sample's size); grid_view: the
    pre-strided view that tap_split hands out, mixed with stride 1 (row and pixel strides carry the factor s)."""
    from dcpt_amd import functional as DF

    idx, n = 1, 3
    full_b = B if form == "dense" else 4
    lo, hi = (0, B) if form == "dense" else (2, 4)
    nb = hi - lo
    big = keyed_input(f"dct.mix.f{B}.{C}.{H}.{s}", (full_b, C, H, W), lo=-1, hi=1)
    prev = keyed_input("dct.mix.p", (nb, C, H // s, W // s), lo=-1, hi=1)
    go = keyed_input("dct.mix.go", (nb, C, H // s, W // s), lo=-1, hi=1)
    mw = keyed_tensor("dct.mixing_weights", (n,))
    # float64 restatement
    b64, p64, m64 = big.double().requires_grad_(True), prev.double().requires_grad_(True), mw.double().requires_grad_(True)
    y64 = (p64 if use_prev else 0) + torch.softmax(m64, 0)[idx] * b64[lo:hi, :, ::s, ::s]
    y64.backward(go.double())
    # HIP
    bg = _nhwc(big.to(dev)).requires_grad_(True)
    pg, mg = _nhwc(prev.to(dev)).requires_grad_(True), mw.to(dev).requires_grad_(True)
    if form == "grid_view":
        y = DF.mix(pg if use_prev else None, bg[lo:hi, :, ::s, ::s], mg, idx)
    else:
        y = DF.mix(pg if use_prev else None, bg[lo:hi] if form == "batch_slice" else bg, mg, idx, stride=s)
    assert tuple(y.shape) == (nb, C, H // s, W // s)
    y.backward(_nhwc(go.to(dev)))
    check("y", y, y64, 1e-5)
    check("dfeat", bg.grad, b64.grad, 1e-5)
    check("dmix", mg.grad, m64.grad, 1e-5)
    if use_prev:
        check("dprev", pg.grad, p64.grad, 1e-5)
    on = torch.zeros(H, W, device=dev)
    on[::s, ::s] = 1.0
    assert float((bg.grad * (1.0 - on)).abs().max()) == 0.0, "positions off the grid get an exactly zero gradient"
    if lo > 0:
        assert float(bg.grad[:lo].abs().max()) == 0.0


def test_stride_1_equals_dense_mix_bit_for_bit_and_backward_repeats(dev):
    from dcpt_amd import functional as DF

    B, C, H, W = 2, 36, 16, 16
    feat = _nhwc(keyed_input("dct.eq.f", (B, C, H, W), lo=-1, hi=1).to(dev))
    prev = _nhwc(keyed_input("dct.eq.p", (B, C, H, W), lo=-1, hi=1).to(dev))
    go = _nhwc(keyed_input("dct.eq.go", (B, C, H, W), lo=-1, hi=1).to(dev))
    mw = keyed_tensor("dct.mixing_weights", (3,)).to(dev)
    for use_prev in (True, False):
        res = []
        for fn in (DF.mix, DF.mix_stride):
            f, p, m = feat.clone().requires_grad_(True), prev.clone().requires_grad_(True), mw.clone().requires_grad_(True)
            y = fn(p if use_prev else None, f, m, 2)
            y.backward(go)
            res.append((y.detach(), f.grad, m.grad))
        for name, a, b in zip(("y", "dfeat", "dmix"), res[0], res[1]):
            assert torch.equal(a, b), f"{name}: dcpt_mix_stride_* at s == 1 on a dense map must equal dcpt_mix_* bit for bit"
    # two runs of the strided backward (SwinIR's width, more than one block of partials): bit-identical, no atomics
    big = _nhwc(keyed_input("dct.rep.f", (2, 180, 32, 32), lo=-1, hi=1).to(dev))
    go2 = _nhwc(keyed_input("dct.rep.go", (2, 180, 16, 16), lo=-1, hi=1).to(dev))
    runs = []
    for _ in range(2):
        f, m = big.clone().requires_grad_(True), mw.clone().requires_grad_(True)
        DF.mix(None, f, m, 1, stride=2).backward(go2)
        runs.append((f.grad, m.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_strided_kernels_refuse_bad_shapes(dev):
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    mw = torch.ones(3, device=dev)
    with pytest.raises(ValueError):
        DF.mix(None, torch.zeros(1, 8, 6, 8, device=dev), mw, 0, stride=4)       # H % s
    with pytest.raises(ValueError):
        DF.mix(None, torch.zeros(1, 8, 8, 8, device=dev), mw, 0, stride=3)       # not a power of two
    with pytest.raises(_lib.DcptHipError):
        DF.mix(None, torch.zeros(1, 6, 8, 8, device=dev), mw, 0, stride=2)       # C % 4 (DCPT_CHECK_ARG)
    with pytest.raises(ValueError):
        DF.tap_split(torch.zeros(2, 8, 6, 8, device=dev), 0, 1, stride=4)


# ---- tap_split(..., stride=s) ----------------------------------------------------------------------------------------------------
class _Probe(torch.autograd.Function):
    """identity; the backward records the gradient that arrives (its address and a copy of its value)"""
    seen = None

    @staticmethod
    def forward(ctx, x):
        return x.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        _Probe.seen = (g.data_ptr(), g.clone())
        return g


class _Fresh(torch.autograd.Function):
    """3 * x; the backward hands on a gradient tensor that nothing else refers to, as the backward of a fused block does"""
    made = None

    @staticmethod
    def forward(ctx, x):
        return x * 3.0

    @staticmethod
    def backward(ctx, go):
        g = go * 3.0
        _Fresh.made = (g.data_ptr(), g.clone())
        return g


def _tap_reference(dev, x, lo, hi, s, mw, idx, gout):
    """the zero-padded gradient of the tap alone (the strided mix on x[lo:hi] of a detached copy: dcpt_grid_scatter + torch's slice)"""
    from dcpt_amd import functional as DF

    xd = x.detach().clone().requires_grad_(True)
    DF.mix(None, xd[lo:hi], mw.detach(), idx, stride=s).backward(gout)
    return xd.grad


@pytest.mark.parametrize("B,C,H,W,s,lo,hi", [(4, 180, 8, 8, 4, 2, 4), (4, 12, 8, 16, 2, 2, 4), (3, 36, 16, 16, 8, 0, 1)])
def test_tap_split_stride_merges_into_a_private_gradient_in_place(dev, B, C, H, W, s, lo, hi):
    from dcpt_amd import functional as DF

    x = _nhwc(keyed_input("dct.ts.x", (B, C, H, W), lo=-1, hi=1).to(dev)).requires_grad_(True)
    mw = keyed_tensor("dct.mixing_weights", (3,)).to(dev).requires_grad_(True)
    gz = _nhwc(keyed_input("dct.ts.gz", (B, C, H, W), lo=-1, hi=1).to(dev))
    gout = _nhwc(keyed_input("dct.ts.go", (hi - lo, C, H // s, W // s), lo=-1, hi=1).to(dev))
    through, tap = DF.tap_split(_Probe.apply(x), lo, hi, stride=s)
    assert tuple(tap.shape) == (hi - lo, C, H // s, W // s) and tap.data_ptr() == x[lo:hi].data_ptr()   # a view: no gather copy
    out = DF.mix(None, tap, mw, 1)
    torch.autograd.backward([_Fresh.apply(through), out], [gz, gout])
    ptr, got = _Probe.seen
    made_ptr, made = _Fresh.made
    assert ptr == made_ptr, "a private main-path gradient is merged in place: the tensor that comes back is the one that went in"
    want = made + _tap_reference(dev, x, lo, hi, s, mw, 1, gout)
    assert torch.equal(got, want), "g + scatter(gs) is an fp32 add of one term: exact"
    assert float((got - made)[lo:hi, :, ::s, ::s].abs().max()) > 0


def test_tap_split_stride_leaves_a_shared_gradient_alone(dev):
    """the consumer is ``a + b``: its backward hands ONE tensor to both inputs, so the merge goes into a copy"""
    from dcpt_amd import functional as DF

    B, C, H, W, s, lo, hi = 4, 12, 8, 8, 2, 2, 4
    x = _nhwc(keyed_input("dct.ts.x", (B, C, H, W), lo=-1, hi=1).to(dev)).requires_grad_(True)
    other = torch.zeros_like(x).requires_grad_(True)
    mw = keyed_tensor("dct.mixing_weights", (3,)).to(dev).requires_grad_(True)
    gz = _nhwc(keyed_input("dct.ts.gz", (B, C, H, W), lo=-1, hi=1).to(dev))
    gz0 = gz.clone()
    gout = _nhwc(keyed_input("dct.ts.go", (hi - lo, C, H // s, W // s), lo=-1, hi=1).to(dev))
    through, tap = DF.tap_split(_Probe.apply(x), lo, hi, stride=s)
    torch.autograd.backward([through + other, DF.mix(None, tap, mw, 1)], [gz, gout])
    assert torch.equal(gz, gz0), "the caller's tensor is unchanged"
    assert torch.equal(other.grad, gz0)
    assert torch.equal(_Probe.seen[1], gz0 + _tap_reference(dev, x, lo, hi, s, mw, 1, gout))
    # no main-path gradient at all: the zero-padded map in one pass
    x2 = x.detach().clone().requires_grad_(True)
    through, tap = DF.tap_split(x2, lo, hi, stride=s)
    DF.mix(None, tap, mw, 1).backward(gout)
    assert torch.equal(x2.grad, _tap_reference(dev, x, lo, hi, s, mw, 1, gout))


# ---- the head against the real reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,dims,nrb", [("a", [12, 12, 12], 1), ("b", [8, 16, 12], 2)])
def test_token_head_golden(dev, golden_dir, tag, dims, nrb):
    """tolerances: those of tests/test_gpu_dchead.py::test_dc_head_golden for the downsample=False head against dc_head.npz"""
    from basicsr.archs import build_network

    g = np.load(os.path.join(golden_dir, "dc_head_tokens.npz"))
    net = build_network(dict(type="PromptIR_NoImg_DC", feature_dims=dims, num_res_blocks=nrb, num_classes=5, downsample=True))
    assert list(net.state_dict().keys()) == [str(k) for k in g[f"{tag}.keys"]]
    fill_module_(net, seed=0)
    net = net.to(dev)
    labels = torch.tensor([3, 1], device=dev)
    res = {}
    for form in ("tokens", "maps"):
        net.zero_grad(set_to_none=True)
        toks = [keyed_input(f"dct.{tag}.f{i}", (2, 256, c), lo=-1.0, hi=1.0).to(dev) for i, c in enumerate(dims)]
        if form == "maps":
            feats = [t.reshape(2, 16, 16, -1).permute(0, 3, 1, 2).requires_grad_(True) for t in toks]
        else:
            feats = [t.requires_grad_(True) for t in toks]
        given = list(feats)
        logits = net(None, given)
        assert all(a is b for a, b in zip(given, feats))
        loss = F.cross_entropy(logits, labels)
        loss.backward()
        dfs = [f.grad if form == "tokens" else f.grad.permute(0, 2, 3, 1).reshape(2, 256, -1) for f in feats]
        res[form] = (logits.detach(), dfs, {k: p.grad.clone() for k, p in net.named_parameters()})
        check("logits", logits, g[f"{tag}.logits"], 1e-4)
        assert abs(float(loss) - float(g[f"{tag}.loss"])) < 1e-5
        for i, d in enumerate(dfs):
            check(f"df{i}", d, g[f"{tag}.df{i}"], 1e-3)
        params = dict(net.named_parameters())
        for n, l2 in zip([str(s) for s in g[f"{tag}.g_names"]], g[f"{tag}.g_l2"]):
            mine = float(params[n].grad.double().pow(2).sum().sqrt())
            assert abs(mine - l2) <= 1e-3 * max(1e-9, l2), (n, mine, l2)
        for k in g.files:
            if k.startswith(f"{tag}.g."):
                check("grad " + k[4:], params[k[4:]].grad, g[k], 1e-3)
    (la, da, pa), (lb, db, pb) = res["tokens"], res["maps"]
    assert torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(da, db)) and all(torch.equal(pa[k], pb[k]) for k in pa)


# ---- the step against the real reference -----------------------------------------------------------------------------------------
def _opt(model_type, batched=True):
    return dict(name="t", model_type=model_type, scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
                hook_names="decode_layers", hook_depth=0, network_g=dict(type="SwinIR", **SWIN_TINY),
                network_dc=dict(type="PromptIR_NoImg_DC", **STEP_HEAD), path=dict(),
                train=dict(pixel_opt=dict(type="L1Loss", loss_weight=1.0, reduction="mean"), batched_encoder_passes=batched,
                           classify_opt=dict(type="CrossEntropyLoss", loss_weight=1.0),
                           optim_g=dict(type="SGD", lr=0.0), optim_dc=dict(type="SGD", lr=0.0)))


def _build(model_type, batched=True):
    from basicsr.models import build_model

    m = build_model(_opt(model_type, batched))
    fill_module_(m.net_g, seed=0)
    fill_module_(m.net_dc, seed=0)
    return m


def _feed(m):
    m.feed_data({"lq": keyed_input("dcsw.lq", (2, 3, 16, 16)), "gt": keyed_input("dcsw.gt", (2, 3, 16, 16)), "dataset_idx": torch.tensor([4, 2])})


@pytest.fixture(scope="module")
def steps(dev):
    """one DCPT step on the tiny SwinIR + token head in both forms (lr 0): (log, logits, gradients)"""
    out = {}
    for batched in (True, False):
        m = _build("DCPTModel", batched)
        assert m.hook_module_names == ["decode_layers0", "decode_layers1", "decode_layers2"] and m.batched_encoder_passes is batched
        _feed(m)
        m.optimize_parameters(1)
        assert m.hook_outputs == []
        out[batched] = (m.get_current_log(), m.cls_output.cpu(), {"g." + k: p.grad.cpu() for k, p in m.net_g.named_parameters()} |
                        {"dc." + k: p.grad.cpu() for k, p in m.net_dc.named_parameters()})
    return out


@pytest.mark.parametrize("batched", [True, False])
def test_swinir_dcpt_step_golden(steps, golden_dir, batched):
    """end-to-end bound (north_star): 1e-3 scale-relative on losses, logits and every gradient"""
    g = np.load(os.path.join(golden_dir, "dcpt_step_swinir.npz"))
    log, logits, grads = steps[batched]
    for k in ("l_pix", "l_classify"):
        e = abs(log[k] - float(g[k])) / abs(float(g[k]))
        print(f"{k}: {log[k]:.7f} vs {float(g[k]):.7f} (relative {e:.3e})")
        assert e <= 1e-3
    check("logits", logits, g["logits"], 1e-3)
    seen = 0
    for k, mine in grads.items():
        tag, name = k.split(".", 1)
        if f"{tag}.g.{name}" in g.files:
            check("grad " + k, mine, g[f"{tag}.g.{name}"], 1e-3)
        else:
            check("grad (every 29th) " + k, mine.flatten()[::SUB], g[f"{tag}.gsub.{name}"], 1e-3)
        seen += 1
    assert seen == len(g["g_names"]) + len(g["dc_names"])
    for tag in ("g", "dc"):
        for n, l2 in zip([str(s) for s in g[f"{tag}_names"]], g[f"{tag}_l2"]):
            mine = float(grads[f"{tag}.{n}"].double().pow(2).sum().sqrt())
            assert abs(mine - l2) <= 1e-3 * max(1e-7, l2), (tag, n, mine, l2)


def test_stacked_pass_equals_two_passes(steps):
    """the bounds of tests/test_gpu_dcpt_step.py::test_batched_encoder_pass_equals_two_passes (NAFNet)"""
    (la, ca, ga), (lb, cb, gb) = steps[True], steps[False]
    assert abs(la["l_pix"] - lb["l_pix"]) < 1e-6 and abs(la["l_classify"] - lb["l_classify"]) < 1e-5
    assert float((ca - cb).abs().max()) <= 1e-5 * float(cb.abs().max())
    for k in gb:
        e = float((ga[k] - gb[k]).abs().max()) / max(1e-7, float(gb[k].abs().max()))
        assert e <= 2e-5, (k, e)


def test_stacked_step_runs_the_strided_kernels(dev):
    from kernel_trace import kernel_trace

    m = _build("DCPTModel", True)
    _feed(m)
    with kernel_trace() as tr:
        m.optimize_parameters(1)
    # three taps: one forward and one backward of the strided mix each (the stride-1 tap is a dense batch slice: the dense kernels), and
    # the two strided taps' gradients merged in place into the main path's
    tr.assert_ran("head.mix_stride_fwd", "head.mix_stride_bwd", "head.grid_add")
    assert tr["head.mix_stride_fwd"] == 2 and tr["head.mix_stride_bwd"] == 2 and tr["head.grid_add"] == 2
    tr.assert_not_ran("head.grid_scatter")
    m2 = _build("DCPTModel", False)
    _feed(m2)
    with kernel_trace() as tr:
        m2.optimize_parameters(1)
    assert tr["head.grid_scatter"] == 2 and tr["head.grid_add"] == 0   # two passes: the zero-padded maps, summed by autograd


class _Loader(list):
    class dataset:   # noqa: N801
        opt = {"name": "synthetic"}


@pytest.mark.parametrize("model_type", ["DCTModel", "DCModel"])
def test_other_model_paths(dev, model_type):
    m = _build(model_type)
    _feed(m)
    m.optimize_parameters(1)
    log = m.get_current_log()
    assert np.isfinite(log["l_classify"]) and m.hook_outputs == []
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.net_dc.parameters())
    if model_type == "DCModel":
        assert all(p.grad is None for p in m.net_g.parameters())
    else:
        assert np.isfinite(log["l_pix"]) and all(p.grad is not None for p in m.net_g.parameters())


def test_validation_returns_top1(dev):
    m = _build("DCPTModel")
    _feed(m)
    m.test()
    assert tuple(m.cls_output.shape) == (2, 5) and m.hook_outputs == []
    data = [{"lq": keyed_input(f"dcsw.val{i}", (1, 3, 16, 24)), "dataset_idx": torch.tensor([i])} for i in range(2)]
    res = m.nondist_validation(_Loader(data), 1, None, False)
    assert 0.0 <= res["top1"] <= 100.0


def test_train_cli_dcpt_swinir():
    """``python basicsr/train.py -opt options/all_in_one/train/train_DCPT_SwinIR_5d.yml`` scaled down through --force_yml"""
    over = ["network_g:embed_dim=36", "network_g:depths=[2,2,2,2,2,2]", "network_dc:feature_dims=[36,36,36]", "network_dc:num_res_blocks=1",
            "datasets:train_1:batch_size_per_gpu=4", "datasets:train_1:gt_size=32", "datasets:train_2:gt_size=32",
            "datasets:train_3:gt_size=32", "datasets:train_1:num=8", "datasets:train_2:num=8", "datasets:train_3:num=8",
            "datasets:val_1:size=32", "train:scheduler:periods=[8]", "logger:print_freq=1", "logger:save_checkpoint_freq=3",
            "val:val_freq=3", "train:optim_g:lr=0.001", "train:optim_dc:lr=0.001", "train:total_iter=3"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    yml = os.path.join(ROOT, "options", "all_in_one", "train", "train_DCPT_SwinIR_5d.yml")
    exp = os.path.join(ROOT, "experiments", "DCPT_SwinIR_5d")
    shutil.rmtree(exp, ignore_errors=True)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "basicsr", "train.py"), "-opt", yml, "--force_yml", *over],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        out = p.stdout + p.stderr
        assert p.returncode == 0, out[-3000:]
        losses = [float(v) for v in re.findall(r"l_classify: ([-0-9.eE+]+)", out)]
        assert len(losses) == 3 and all(0.0 < v < 20.0 for v in losses), out[-2000:]
        assert "# top1:" in out and os.path.exists(os.path.join(exp, "models", "net_dc_3.pth"))
        assert os.path.exists(os.path.join(exp, "models", "net_g_3.pth"))
    finally:
        shutil.rmtree(exp, ignore_errors=True)
