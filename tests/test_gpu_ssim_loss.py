"""GPU: the SSIM losses on the fused fp64 kernels (dcpt_amd/csrc/ssim_loss.hip through DF.ssim_pt, basicsr.metrics.calculate_ssim_pt,
SSIMLoss / SSIMMSELoss) against tests/ssim_restatement.py, the kernel-blind float64 restatement of the reference on the CPU.

Bounds (set by the arithmetic, not tuned):
* SSIM per image: 1e-10 absolute -- SSIM_TOL of tests/test_gpu_metrics.py, derived there for values up to 255^2; range 1 is easier.
  Identical images: 1 within 1e-12.
* Gradient, every element: |g - T| <= 2^-23 |T| + 1e-9 max|T|.  The first term is the one fp32 rounding of the result with one ulp of slack,
  the second caps what another order of the fp64 sums can move (the closed form against autograd: ~1e-14 relative, test_ssim_loss_cpu.py).
  T for ``ssim_pt`` is the float64 autograd gradient of the restatement (a float64 leaf holding the fp32 values).
* Identical and all-zero images: |g| <= 1e-9.
* Loss classes: the value by the first rule, ``pred.grad`` by the second; T from an fp32 leaf, as the classes are used.

Every case prints its worst figure as a ratio to its bound before it asserts.  Measured on the MI355X: SSIM within 1.6e-15 of the
restatement, the worst gradient element at 0.48 of its bound, |g| <= 2.8e-17 on identical images and exactly 0 on zero images, the loss
classes' values within 2.1e-17 and their ``pred.grad`` equal to the restatement's bit for bit."""
import pytest
import torch

import ssim_restatement as R
from dcpt_amd.keyed_init import keyed_input

pytestmark = pytest.mark.gpu
SSIM_TOL = 1e-10
TH, TW = 16, 32   # DF.METRIC_TILE: map positions per workgroup of the tile kernels, input pixels per workgroup of the gather kernel
# (B, C, H, W), crop_border, test_y_channel -- and what the shape is there for
CASES = {
    "one_position": ((1, 1, 11, 11), 0, False),            # each pixel has one tap
    "one_tile": ((2, 3, TH + 10, TW + 10), 0, False),      # exactly one tile of map positions
    "past_tile": ((1, 3, TH + 11, TW + 11), 0, False),     # one position past the tile in each axis
    "ragged_crop": ((2, 3, 40, 75), 3, False),             # several ragged tiles; the border gradient must be bitwise 0
    "luma": ((1, 3, 33, 21), 0, True),
    "luma_crop": ((2, 3, 30, 45), 2, True),                # luma with a border and a second image
    "gray": ((3, 1, 12, 50), 0, False),                    # single-channel images (the luma flag would do nothing)
    "gray_luma_flag": ((2, 1, 13, 23), 1, True),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    _lib.load()
    assert DF.METRIC_TILE == (TH, TW)
    return torch.device("cuda:0")


def _inputs(name, kind):
    shape = CASES[name][0] if name in CASES else name
    if kind == "zero":
        return torch.zeros(shape), torch.zeros(shape)
    pred = keyed_input(f"gpussim.{name}.a", shape)
    if kind == "same":
        return pred, pred.clone()
    return pred, (pred + keyed_input(f"gpussim.{name}.n", shape, lo=-0.08, hi=0.08)).clamp(0, 1)


def _upstream(B):
    """the weight of each image's SSIM in the scalar that is differentiated: different per image, one negative"""
    return torch.tensor([1.0, -0.5, 2.0, 0.75, 1.5, -1.25, 0.25][:B], dtype=torch.float64)


_REF = {}


def _reference(name, kind):
    """(per-image SSIM, float64 gradient of sum_b upstream[b] ssim[b]) of the restatement: computed once per case and shared"""
    if (name, kind) not in _REF:
        shape, crop, y = CASES[name]
        pred, target = _inputs(name, kind)
        leaf = pred.double().requires_grad_(True)
        s = R.ssim_pt(leaf, target.double(), crop, y, 1.0)
        (s * _upstream(shape[0])).sum().backward()
        _REF[name, kind] = (s.detach(), leaf.grad)
    return _REF[name, kind]


def _grad_ratio(g, T):
    """the worst |g - T| as a ratio to the bound 2^-23 |T| + 1e-9 max|T|"""
    T = T.double()
    bound = 2.0 ** -23 * T.abs() + 1e-9 * float(T.abs().max())
    return float(((g.double() - T).abs() / bound.clamp_min(1e-300)).max())


def _run(name, kind, dev):
    from dcpt_amd import functional as DF

    shape, crop, y = CASES[name]
    pred, target = _inputs(name, kind)
    p = pred.to(dev).requires_grad_(True)
    s = DF.ssim_pt(p, target.to(dev), crop, y, 1.0)
    (s * _upstream(shape[0]).to(dev)).sum().backward()
    return s.detach().cpu(), p.grad.cpu()


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradient_match_the_restatement(name, dev):
    shape, crop, y = CASES[name]
    s, g = _run(name, "noisy", dev)
    Ts, Tg = _reference(name, "noisy")
    assert s.dtype == torch.float64 and tuple(s.shape) == (shape[0],) and g.dtype == torch.float32 and tuple(g.shape) == shape
    dv, ratio = float((s - Ts).abs().max()), _grad_ratio(g, Tg)
    print(f"ssim_pt {name} {shape} crop {crop} y {int(y)}: ssim {[float(v) for v in Ts]} |d| {dv:.3e} (bound 1e-10); "
          f"gradient max|T| {float(Tg.abs().max()):.3e} worst ratio to the bound {ratio:.3f}")
    assert float(Tg.abs().max()) > 1e-4 and float(Ts.max()) < 0.9999
    assert dv <= SSIM_TOL
    assert ratio <= 1.0
    if crop:   # bitwise +0 in the border, and something inside it
        inner = torch.zeros(shape, dtype=torch.bool)
        inner[:, :, crop:-crop, crop:-crop] = True
        assert int(g[~inner].view(torch.int32).abs().max()) == 0 and float(g[inner].abs().min()) > 0


@pytest.mark.parametrize("kind", ["same", "zero"])
@pytest.mark.parametrize("name", ["past_tile", "ragged_crop", "luma", "gray"])
def test_identical_and_zero_images(name, kind, dev):
    s, g = _run(name, kind, dev)
    Ts, Tg = _reference(name, kind)
    print(f"ssim_pt {name} {kind}: max|ssim - 1| {float((s - 1).abs().max()):.3e} (bound 1e-12) max|g| {float(g.abs().max()):.3e} (bound 1e-9; "
          f"restatement {float(Tg.abs().max()):.3e})")
    assert float((s - 1).abs().max()) <= 1e-12 and float((s - Ts).abs().max()) <= SSIM_TOL
    assert float(g.abs().max()) <= 1e-9 and float(Tg.abs().max()) <= 1e-9


def test_more_images_than_one_backward_chunk(dev):
    """5 images under a plane cap that holds 2: three chunks (2, 2, 1), the same bits as one chunk, and the restatement's values"""
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    shape = (5, 3, 14, 15)
    pred, target = _inputs(shape, "noisy")
    up = _upstream(5)

    def grad():
        p = pred.to(dev).requires_grad_(True)
        (DF.ssim_pt(p, target.to(dev)) * up.to(dev)).sum().backward()
        return p.grad.cpu()

    whole = grad()
    cap = DF.ssim_plane_cap()
    per = 3 * 24 * 4 * 5
    try:
        DF.ssim_plane_cap(2 * per + 7)
        with kernel_trace() as t:
            chunked = grad()
    finally:
        DF.ssim_plane_cap(cap)
    assert t["ssim_loss.tile_bwd"] == 3 and t["ssim_loss.gather"] == 3 and t["ssim_loss.tile_fwd"] == 1
    assert torch.equal(whole.view(torch.int32), chunked.view(torch.int32))
    leaf = pred.double().requires_grad_(True)
    (R.ssim_pt(leaf, target.double()) * up).sum().backward()
    ratio = _grad_ratio(chunked, leaf.grad)
    print(f"ssim_pt chunks {shape}: worst ratio to the bound {ratio:.3f}")
    assert ratio <= 1.0


def _loss_pair(cls, fn, kw, pred, target, dev, weight=None):
    """(value, pred.grad) of the class on the device and of the restatement on the CPU, fp32 leaves on both sides"""
    import basicsr.losses as L

    p = pred.to(dev).requires_grad_(True)
    args = (p, target.to(dev)) + ((weight.to(dev),) if weight is not None else ())
    v = getattr(L, cls)(**kw)(*args)
    v.backward()
    q = pred.clone().requires_grad_(True)
    T = fn(q, target, *((weight,) if weight is not None else ()), **kw)
    T.backward()
    return v.detach().cpu(), p.grad.cpu(), T.detach(), q.grad


LOSS_CASES = [
    ("SSIMLoss", dict(), (3, 3, 27, 43), None),
    ("SSIMLoss", dict(ssim_weight=0.3, mse_weight=2.0, crop_border=3, reduction="sum"), (2, 3, 40, 45), "w3"),
    ("SSIMLoss", dict(test_y_channel=True, crop_border=1), (2, 3, 30, 24), "w1"),
    ("SSIMMSELoss", dict(), (3, 3, 27, 43), None),
    ("SSIMMSELoss", dict(ssim_weight=0.5, mse_weight=0.25, crop_border=2, reduction="sum", test_y_channel=True), (2, 3, 31, 50), None),
    ("SSIMMSELoss", dict(crop_border=1), (2, 1, 20, 36), None),
]


@pytest.mark.parametrize("cls, kw, shape, wkind", LOSS_CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(LOSS_CASES)])
def test_loss_classes_match_the_restatement(cls, kw, shape, wkind, dev):
    pred, target = _inputs(shape, "noisy")
    weight = None if wkind is None else keyed_input(f"gpussim.{wkind}", (shape[0], 3 if wkind == "w3" else 1, shape[2], shape[3]))
    fn = R.ssim_loss if cls == "SSIMLoss" else R.ssim_mse_loss
    v, g, T, Tg = _loss_pair(cls, fn, kw, pred, target, dev, weight)
    assert v.dtype == torch.float64 and v.dim() == 0 and T.dtype == torch.float64 and g.dtype == torch.float32
    ratio = _grad_ratio(g, Tg)
    print(f"{cls} {kw} {shape} weight {wkind}: value {float(T)!r} |d| {abs(float(v) - float(T)):.3e} (bound 1e-10); gradient max|T| "
          f"{float(Tg.abs().max()):.3e} worst ratio to the bound {ratio:.3f}")
    assert abs(float(v) - float(T)) <= SSIM_TOL
    assert ratio <= 1.0
    if cls == "SSIMLoss":   # the [0]: images 1.. get the Huber term's gradient alone
        q = pred.clone().requires_grad_(True)
        (kw.get("mse_weight", 1.0) * R.huber_loss(q, target, weight, kw.get("reduction", "mean"))).backward()
        assert _grad_ratio(g[1:], q.grad[1:]) <= 1.0 and not torch.equal(g[:1], q.grad[:1])


def test_metric_entry_and_argument_checks(dev):
    from basicsr.metrics import calculate_ssim_pt
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    pred, target = (t.to(dev) for t in _inputs((2, 3, 20, 24), "noisy"))
    # the registered metric: the reference's default image_range 255 on [0, 1] images (C1, C2 scale with it)
    got = calculate_ssim_pt(pred, target, 2, test_y_channel=True).cpu()
    want = R.ssim_pt(pred.cpu(), target.cpu(), 2, True, 255)
    assert float((got - want).abs().max()) <= SSIM_TOL and float((got - R.ssim_pt(pred.cpu(), target.cpu(), 2, True, 1.0)).abs().max()) > 1e-3
    with pytest.raises(NotImplementedError):
        DF.ssim_pt(pred, target.clone().requires_grad_(True))
    with pytest.raises(_lib.DcptHipError, match="fp32"):
        DF.ssim_pt(pred.double(), target.double())
    with pytest.raises(_lib.DcptHipError, match="no CPU fallback"):
        DF.ssim_pt(pred, target.cpu())
    with pytest.raises(ValueError):
        DF.ssim_pt(pred, target[:, :, :-1])
    with pytest.raises(ValueError):
        DF.ssim_pt(pred[0], target[0])
    with pytest.raises(_lib.DcptHipError, match="at least 11 x 11"):
        DF.ssim_pt(pred, target, 5)
    with pytest.raises(_lib.DcptHipError, match="C must be 1 or 3"):
        DF.ssim_pt(pred[:, :2], target[:, :2])
    with pytest.raises(_lib.DcptHipError, match="image_range"):
        DF.ssim_pt(pred, target, image_range=0.0)
    with pytest.raises(_lib.DcptHipError, match="crop_border"):
        DF.ssim_pt(pred, target, -1)


def test_two_runs_give_identical_bits_and_noncontiguous_inputs_are_taken(dev):
    from dcpt_amd import functional as DF

    pred, target = (t.to(dev) for t in _inputs((2, 3, 2 * TH + 13, 2 * TW + 13), "noisy"))

    def run(a, b, y):
        a = a.detach().requires_grad_(True)
        s = DF.ssim_pt(a, b, 1, y)
        (s * _upstream(2).to(dev)).sum().backward()
        return s.detach(), a.grad

    for y in (False, True):
        s1, g1 = run(pred, target, y)
        s2, g2 = run(pred, target, y)
        assert torch.equal(s1.view(torch.int64), s2.view(torch.int64)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
        # a channels_last tensor / a sliced view of a larger one: .contiguous() inside, the same bits out, the gradient in pred's shape
        s3, g3 = run(pred.contiguous(memory_format=torch.channels_last), torch.cat([target, target], 3)[..., : target.shape[3]], y)
        assert torch.equal(s1.view(torch.int64), s3.view(torch.int64)) and torch.equal(g1.view(torch.int32), g3.contiguous().view(torch.int32))


def test_stays_inside_its_buffers_and_refuses_a_short_workspace(dev):
    """the entry points on buffers of exactly the size they ask for, with guards behind ssim_sum, dpred and the workspace (all of them
    start as NaN patterns: nothing unwritten is read); then one byte less: refused, nothing launched"""
    from kernel_trace import kernel_trace
    from redzone import redzone

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    for (B, C, H, W), crop, y in (((3, 3, TH + 11 + 6, TW + 9 + 6), 3, False), ((2, 3, TH + 12, TW + 13), 0, True)):
        pred, target = (t.to(dev) for t in _inputs((B, C, H, W), "noisy"))
        dims, cp = (B, C, H, W, crop, int(y)), (1 if y else C)
        p = pred.clone().requires_grad_(True)
        s = DF.ssim_pt(p, target, crop, y)
        up = _upstream(B).to(dev)
        (s * up).sum().backward()
        count = cp * (H - 2 * crop - 10) * (W - 2 * crop - 10)
        gscale = (up / count).reshape(-1, 1).expand(-1, cp).contiguous()
        nf, nb = lib.dcpt_ssim_loss_ws_bytes(*dims, 0), lib.dcpt_ssim_loss_ws_bytes(*dims, 1)
        with redzone() as rz:
            sums = DF._workspace(dev, B * cp * 8)
            dpred = DF._workspace(dev, B * C * H * W * 4)
            wf, wb = DF._workspace(dev, nf), DF._workspace(dev, nb)
            DF._call(lib.dcpt_ssim_loss_fwd, (pred, target, sums, wf, nf), (*dims, 1.0), dev)
            DF._call(lib.dcpt_ssim_loss_bwd, (pred, target, gscale, dpred, wb, nb), (*dims, 1.0), dev)
        assert rz.count == 4
        assert torch.equal((sums.view(torch.float64).view(B, cp).sum(1) / count).view(torch.int64), s.detach().view(torch.int64))
        assert torch.equal(dpred.view(torch.int32), p.grad.reshape(-1).view(torch.int32))
        with kernel_trace() as t:
            rc_f = lib.dcpt_ssim_loss_fwd(pred.data_ptr(), target.data_ptr(), sums.data_ptr(), wf.data_ptr(), nf - 1, *dims, 1.0, None)
            err_f = lib.dcpt_last_error()
            rc_b = lib.dcpt_ssim_loss_bwd(pred.data_ptr(), target.data_ptr(), gscale.data_ptr(), dpred.data_ptr(), wb.data_ptr(), nb - 1, *dims, 1.0,
                                          None)
            err_b = lib.dcpt_last_error()
        assert rc_f == 2 and rc_b == 2 and b"workspace too small" in err_f and b"workspace too small" in err_b
        assert t.counts == {}


def test_launch_trace_names_the_ssim_loss_kernels(dev):
    from kernel_trace import kernel_trace

    from dcpt_amd import functional as DF

    pred, target = (t.to(dev) for t in _inputs((2, 3, 24, 24), "noisy"))
    with kernel_trace() as t:
        p = pred.requires_grad_(True)
        DF.ssim_pt(p, target).sum().backward()
    t.assert_ran("ssim_loss.tile_fwd", "ssim_loss.reduce", "ssim_loss.tile_bwd", "ssim_loss.gather")
    assert set(t.families()) == set(t.families("ssim_loss.")) and all(v == 1 for v in t.counts.values())


def test_training_step_with_ssim_loss(dev):
    """one SRModel.optimize_parameters step of a tiny NAFNetBaseline under pixel_opt SSIMLoss: it runs, logs a finite l_pix and moves the
    parameters; the float64 loss passes reduce_loss_dict and the pending log"""
    import math

    from basicsr.models import build_model
    from dcpt_amd.keyed_init import fill_module_

    tiny = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1])
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
               network_g=dict(type="NAFNetBaseline", window_size=16, **tiny), path=dict(pretrain_network_g=None),
               train=dict(pixel_opt=dict(type="SSIMLoss", ssim_weight=0.5, crop_border=1), optim_g=dict(type="SGD", lr=0.05)))
    m = build_model(opt)
    fill_module_(m.net_g)
    before = [p.detach().clone() for p in m.net_g.parameters()]
    gt, lq = _inputs((2, 3, 32, 32), "noisy")
    m.feed_data({"lq": lq, "gt": gt})
    m.optimize_parameters(1)
    log = m.get_current_log()
    print(f"SRModel step with SSIMLoss: l_pix {log['l_pix']!r}")
    assert isinstance(log["l_pix"], float) and math.isfinite(log["l_pix"]) and log["l_pix"] > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.net_g.parameters())
    assert sum(int(not torch.equal(a, b.detach())) for a, b in zip(before, m.net_g.parameters())) > len(before) // 2
