"""GPU tests of the TLSC (local-mean SCA) NAFBlock in bf16 storage: dcpt_nafblock_local_fwd_bf16, its box-mean kernels
(dcpt_amd/csrc/tlsc_bf16.hip, also through the thin entry point dcpt_box_mean_bf16) and the EB_MUL epilogue of the bf16 NT GEMM, up to
``NAFNet(act_dtype="bf16" | "bf16_tail32" | "bf16_edge32")`` and tiled inference.

Tolerances, stated up front.
  * block vs the fp32 TLSC block (DF.nafblock_local, same bf16-representable input, fp32 parameters): the constant and metric that
    tests/test_gpu_bf16.py::test_nafblock_bf16_oracle applies to nafblock_bf16 against its fp32 yardstick -- max |a - b| / max |b| <= 4e-2.
  * network vs tests/golden/nafnet_local_tiny.npz (the real reference's TLSC output): what tests/test_gpu_bf16.py::test_nafnet_bf16_end_to_end
    allows the bf16 NAFNetBaseline against the fp32 network's output, 3e-2 in the same metric.  TINY's width is 8, so no width-8 twin is needed.
  * box mean vs a float64 unfold mean + replicate pad of the same bf16 inputs: one bf16 rounding,
    |d| <= 2^-8 |ref| + k1 k2 2^-24 mean|x|  (the second term bounds the fp32 accumulation).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import keyed_input, keyed_state_dict, keyed_tensor
from oracle import nafnet_oracle as O

pytestmark = pytest.mark.gpu

BLOCK_TOL = 4e-2   # tests/test_gpu_bf16.py:137  (_rel(yd, yf) <= 4e-2)
NET_TOL = 3e-2     # tests/test_gpu_bf16.py:349  (bf16 network vs the fp32 network's output)
TINY = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 2], dec_blk_nums=[1, 1, 1, 1])   # tests/test_gpu_parity.py
FUSED = {"norm1_w": "norm1.weight", "norm1_b": "norm1.bias", "conv1_w": "conv1.weight", "conv1_b": "conv1.bias",
         "conv2_w": "conv2.weight", "conv2_b": "conv2.bias", "conv3_w": "conv3.weight", "conv3_b": "conv3.bias",
         "sca_w": "sca.1.weight", "sca_b": "sca.1.bias", "norm2_w": "norm2.weight", "norm2_b": "norm2.bias",
         "conv4_w": "conv4.weight", "conv4_b": "conv4.bias", "conv5_w": "conv5.weight", "conv5_b": "conv5.bias",
         "beta": "beta", "gamma": "gamma"}
# (H, W), (k1, k2): even windows and M = 99; M = 480, a ragged last tile; Ho = 1; the mean map equals t2
CASES = [((1, 9, 11), (4, 6)), ((2, 12, 20), (5, 5)), ((1, 8, 16), (8, 3)), ((1, 6, 10), (1, 1))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def widths(dev):
    """one width from each class of dcpt_nafblock_bf16_fused_ffn (1: one kernel for the second half, 2: the chain kernel, 0: neither), queried"""
    from dcpt_amd import _lib

    lib = _lib.load()
    first = {}
    for c in (16, 32, 64, 128, 256, 512):
        first.setdefault(int(lib.dcpt_nafblock_bf16_fused_ffn(c)), c)
    assert set(first) == {0, 1, 2}, first
    return [first[1], first[2], first[0]]


def _rel(a, b):
    a, b = a.detach().float().cpu().double(), b.detach().float().cpu().double()
    assert a.shape == b.shape
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _params(c, prefix, dev):
    full = O.nafnet_param_shapes(width=c, enc_blk_nums=[1], middle_blk_num=0, dec_blk_nums=[])
    P = {k[len("encoders.0.0."):]: keyed_tensor(prefix + k[len("encoders.0.0."):], s) for k, s in full.items() if k.startswith("encoders.0.0.")}
    return {k: P[v].to(dev) for k, v in FUSED.items()}


def _input(tag, shape, dev):
    x = keyed_input(tag, shape, lo=-1.5, hi=1.5).bfloat16().float()   # bf16-representable
    return x.to(dev).contiguous(memory_format=torch.channels_last)


_REF = {}   # (c, shape, k) -> (parameters, fp32 input, fp32 TLSC output): computed once, shared, never changed


def _reference(dev, c, bhw, k):
    from dcpt_amd import functional as DF

    key = (c, bhw, k)
    if key not in _REF:
        B, H, W = bhw
        tag = f"tlscbf.{c}.{H}x{W}."
        P = _params(c, tag, dev)
        x = _input(tag + "x", (B, c, H, W), dev)
        with torch.no_grad():
            _REF[key] = (P, x, DF.nafblock_local(x, P, *k))
    return _REF[key]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("cls", [0, 1, 2])
def test_block_vs_fp32_tlsc_block_and_kernel_selection(dev, widths, cls, case):
    """1 + 2: nafblock_local_bf16 against the fp32 TLSC block; the call launched the bf16 box mean and an EB_MUL GEMM, and neither the
    global pooling's finisher (sca_fwd) nor the fp32 box mean."""
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    c = widths[cls]
    bhw, k = CASES[case]
    P, x, yf = _reference(dev, c, bhw, k)
    with torch.no_grad(), kernel_trace() as tr:
        yb = DF.nafblock_local_bf16(x.bfloat16(), P, *k)
        torch.cuda.synchronize()
    assert yb.dtype == torch.bfloat16 and yb.shape == x.shape
    e = _rel(yb, yf)
    print(f"C={c} {bhw} k={k}: rel err vs fp32 TLSC block {e:.4e}")
    tr.assert_ran("tlsc.box_mean_bf16", "nt_bf16.epi_mul")
    tr.assert_not_ran("sca_fwd", "tlsc.box_mean_f32")
    assert tr["tlsc.box_mean_bf16"] == 1 and tr["nt_bf16.epi_mul"] == 1, tr.counts
    assert np.isfinite(e) and e <= BLOCK_TOL, (c, bhw, k, e)
    if k == (1, 1):   # the pack given by the caller changes no bit
        pk = DF.PackedWeightsBf16()
        with torch.no_grad():
            assert torch.equal(DF.nafblock_local_bf16(x.bfloat16(), P, *k, packed=pk), yb)


# the multiply epilogue on the two large tile classes of the bf16 NT GEMM: the dispatcher takes them from 192 tiles on, i.e. 512 x 128 tiles
# at N = K = 128 from M = 191 * 512 + 1 = 97793 rows and 256 x 256 tiles at N = K = 256 from M = 191 * 256 + 1 = 48897 rows (what NAFNet-64 TLSC
# runs at levels 1 and 2 of a 2K image or a 512 tile).  M = 221 * 443 = 97903 leaves 111 rows in the last 512-row tile (three of its four
# 128-row parts empty, the first ragged), M = 111 * 441 = 48951 leaves 55 in the last 256-row tile (its second half empty): M % 256 in [1, 128].
BIG_TILE_CASES = [(128, (1, 221, 443), (37, 60), "nt_bf16.epi_mul.tall512"), (256, (1, 111, 441), (20, 33), "nt_bf16.epi_mul.256")]


@pytest.mark.parametrize("c,bhw,k,family", BIG_TILE_CASES)
def test_mul_epilogue_on_the_large_tiles(dev, c, bhw, k, family):
    """EB_MUL on the 512 x 128 and 256 x 256 tiles with a ragged last tile, through the block, against the fp32 TLSC block at test 1's bound;
    output and workspace start as NaN under red zones, so a row the last tile failed to write, or wrote past the end, is seen."""
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace
    from redzone import redzone

    B, H, W = bhw
    M = B * H * W
    assert 1 <= M % (512 if family.endswith("tall512") else 256) <= 128   # the last tile holds one ragged 128-row part, the rest is empty
    P, x, yf = _reference(dev, c, bhw, k)
    with torch.no_grad(), kernel_trace() as tr, redzone() as rz:
        yb = DF.nafblock_local_bf16(x.bfloat16(), P, *k)
    assert rz.count >= 2
    assert tr["nt_bf16.epi_mul"] == 1 and tr[family] == 1 and tr["tlsc.box_mean_bf16"] == 1, tr.counts
    assert bool(torch.isfinite(yb.float()).all())
    e = _rel(yb, yf)
    tail = M % 256   # the rows of the last tile on their own (NHWC: the last pixels of the map)
    fl = lambda t: t.permute(0, 2, 3, 1).reshape(M, c)[M - tail:]
    et = float((fl(yb).float() - fl(yf)).abs().max() / yf.abs().max())
    print(f"C={c} {bhw} k={k} {family}: rel err vs fp32 TLSC block {e:.4e}, in the last tile's {tail} rows {et:.4e}")
    assert np.isfinite(e) and e <= BLOCK_TOL, (c, bhw, k, e)


def test_window_edge(dev, widths):
    """3: the local entry point with k = (H, W) -- one window, the global mean -- against nafblock_bf16 on the same input; through
    NAFBlock.forward a window that covers the map still dispatches to the global block."""
    from basicsr.archs.arch_util import AvgPool2d
    from basicsr.archs.nafnet_arch import NAFBlock
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace

    for c in widths:
        (B, H, W), _ = CASES[1]
        P, x, _ = _reference(dev, c, CASES[1][0], CASES[1][1])
        with torch.no_grad():
            yl = DF.nafblock_local_bf16(x.bfloat16(), P, H, W)
            yg = DF.nafblock_bf16(x.bfloat16(), P)
        e = _rel(yl, yg)
        print(f"C={c}: local k=(H,W) vs global bf16 block {e:.4e}")
        assert np.isfinite(e) and e <= BLOCK_TOL, (c, e)
    c = widths[0]
    blk = NAFBlock(c).to(dev).eval()
    blk.act_bf16 = True
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(keyed_tensor("tlscbf.edge." + str(tuple(p.shape)), tuple(p.shape)).to(dev))
    blk.sca[0] = AvgPool2d(kernel_size=[12, 20])
    x = _input("tlscbf.edge.x", (1, c, 12, 20), dev)
    with torch.no_grad(), kernel_trace() as tr:
        blk(x)
        torch.cuda.synchronize()
    tr.assert_ran("sca_fwd")
    tr.assert_not_ran("tlsc.box_mean_bf16", "nt_bf16.epi_mul")
    x = _input("tlscbf.edge.x2", (1, c, 12, 21), dev)   # one column more than the window: local
    with torch.no_grad(), kernel_trace() as tr:
        blk(x)
        torch.cuda.synchronize()
    tr.assert_ran("tlsc.box_mean_bf16", "nt_bf16.epi_mul")


def test_workspace_bounds(dev, widths):
    """4: exactly dcpt_nafblock_local_fwd_bf16_ws_bytes is enough (guards behind the workspace and the output intact, and no NaN from
    workspace that was never written); one byte less returns DCPT_ERR_WS and launches nothing."""
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace
    from redzone import redzone

    lib = _lib.load()
    c = max(widths)
    (B, H, W), k = CASES[1]
    P, x, yf = _reference(dev, c, (B, H, W), k)
    xb = x.bfloat16()
    with torch.no_grad(), redzone() as rz:
        y = DF.nafblock_local_bf16(xb, P, *k)
    assert rz.count >= 2
    assert bool(torch.isfinite(y.float()).all()) and _rel(y, yf) <= BLOCK_TOL
    need = int(lib.dcpt_nafblock_local_fwd_bf16_ws_bytes(B, H, W, c, *k))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full_like(xb, 7.0)
    ps = [P[f].contiguous() for f in _lib.PARAM_FIELDS]
    pp = _lib.NafBlockParams(*[p.data_ptr() for p in ps])
    with kernel_trace() as tr:
        rc = lib.dcpt_nafblock_local_fwd_bf16(C.byref(pp), None, 0, xb.data_ptr(), out.data_ptr(), ws.data_ptr(), need - 1, B, H, W, c, k[0], k[1],
                                              torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
    assert rc == 2, rc   # DCPT_ERR_WS
    assert tr.counts == {}, tr.counts
    assert bool((out.float() == 7.0).all())


@pytest.fixture(scope="module")
def tlsc_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "nafnet_local_tiny.npz"))["y"]


def _tlsc_net(dev, mode):
    from basicsr.archs import build_network

    net = build_network(dict(type="NAFNet", train_size=(1, 3, 16, 16), act_dtype=mode, **TINY))
    net.load_state_dict(keyed_state_dict(O.nafnet_param_shapes(**TINY), seed=0), strict=True)
    return net.to(dev).eval()


@pytest.mark.parametrize("mode", ["bf16", "bf16_tail32", "bf16_edge32"])
def test_network_vs_reference_golden(dev, tlsc_golden, mode):
    """5: NAFNet (TLSC) in the three bf16 storage modes on the input of test_nafnet_local_tlsc_golden against the real reference's output;
    the trace says which groups ran the bf16 local block and which the fp32 one.  (Raises NotImplementedError without the feature.)
    6: inference only, as in fp32."""
    from kernel_trace import kernel_trace

    net = _tlsc_net(dev, mode)
    x = keyed_input("tlsc.img", (1, 3, 48, 32)).to(dev)
    with torch.no_grad(), kernel_trace() as tr:
        y = net(x)
        torch.cuda.synchronize()
    e = _rel(y, torch.from_numpy(tlsc_golden))
    print(f"{mode}: rel err vs the reference's TLSC output {e:.4e}")
    # every block of this net on this input has a window smaller than its map (24 x 24 on 48 x 32 ... 1 x 1 on 3 x 2): ten local blocks;
    # bf16_tail32 keeps the last decoder group (one block) in fp32, bf16_edge32 the first encoder group (one block) as well
    n32 = {"bf16": 0, "bf16_tail32": 1, "bf16_edge32": 2}[mode]
    assert sum(1 for m in net.modules() if hasattr(m, "local_sca") and m.local_sca()) == 10
    assert tr["tlsc.box_mean_bf16"] == 10 - n32 and tr["nt_bf16.epi_mul"] == 10 - n32 and tr["tlsc.box_mean_f32"] == n32, tr.counts
    # the TLSC blocks in bf16 storage are in the network's weight-pack list (they read the global block's pack), the fp32 ones are not
    assert len(net._bf16_blocks) == 10 - n32 and all(m.local_sca() and m.act_bf16 and m._packed_bf16 is not None for m in net._bf16_blocks)
    want32 = [m for m in list(getattr(net, "decoder3")) * (n32 >= 1) + list(net.encoders[0]) * (n32 >= 2)]
    assert [m for m in net.modules() if hasattr(m, "local_sca") and not m.act_bf16] == [m for m in net.modules() if any(m is q for q in want32)]
    assert y.dtype == torch.float32 and np.isfinite(e) and e <= NET_TOL, (mode, e)
    with pytest.raises(NotImplementedError):
        net(x.requires_grad_(True))


def test_tiles(dev):
    """7: SRModel.test_tile with a TLSC bf16 net on a 40 x 56 image, infer_size 32, tile_pad 4, equals the per-tile loop (the check of
    tests/test_gpu_parity.py::test_tiled_inference_matches_per_tile_loop).  The padded tiles are 36 or 12 rows by 36 or 28 columns, so
    the net has two down layers (every tile side a multiple of 4); its level-0 window is 24 x 24: inside the 36-pixel tiles, clamped to
    12 rows in the bottom ones."""
    from basicsr.models import build_model

    cfg = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1], dec_blk_nums=[1, 1])
    opt = dict(name="t", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="NAFNet", train_size=(1, 3, 16, 16), act_dtype="bf16", window_size=4, **cfg), path=dict(),
               tile=dict(infer_size=32, tile_pad=4), val=dict(save_img=False))
    m = build_model(opt)
    m.net_g.load_state_dict(keyed_state_dict(O.nafnet_param_shapes(**cfg), seed=0), strict=True)
    img = keyed_input("tlscbf.tile.img", (1, 3, 40, 56))
    m.feed_data({"lq": img})
    m.pre_test()
    Hp, Wp = m.lq.shape[-2:]
    assert (Hp, Wp) == (40, 56)
    m.test_tile()
    m.post_test()
    got = m.output.cpu()
    lq = F.pad(img, (0, Wp - 56, 0, Hp - 40), "reflect").to(dev)
    ref = torch.zeros_like(lq)
    with torch.no_grad():
        for y0 in range(0, Hp, 32):
            for x0 in range(0, Wp, 32):
                x1, y1 = min(x0 + 32, Wp), min(y0 + 32, Hp)
                xp0, yp0, xp1, yp1 = max(x0 - 4, 0), max(y0 - 4, 0), min(x1 + 4, Wp), min(y1 + 4, Hp)
                out = m.net_g(lq[:, :, yp0:yp1, xp0:xp1].contiguous())
                ref[:, :, y0:y1, x0:x1] = out[:, :, y0 - yp0:y0 - yp0 + (y1 - y0), x0 - xp0:x0 - xp0 + (x1 - x0)]
    ref = ref[:, :, :40, :56].cpu()
    e = float((got - ref).abs().max() / ref.abs().max())
    print(f"tiled vs per-tile loop: {e:.3e}")
    assert got.shape == ref.shape and e <= 1e-5, e


# ---- the box mean's index arithmetic on its own (dcpt_box_mean_bf16) -------------------------------------------------------------
def _box_mean_f64(x, k1, k2):
    """arch_util.py:378-396 in float64: unfold mean over the valid windows, replicate pad back, the smaller pad on the left / top"""
    B, c, H, W = x.shape
    xd = x.double()
    m = F.unfold(xd.reshape(B * c, 1, H, W), (k1, k2)).mean(1).reshape(B, c, H - k1 + 1, W - k2 + 1)
    ph, pw = H - m.shape[2], W - m.shape[3]
    return F.pad(m, (pw // 2, (pw + 1) // 2, ph // 2, (ph + 1) // 2), mode="replicate")


# windows of the block test + more than one chunk along both axes (a chunk is >= 8 outputs, >= k2 / 4 columns, >= k1 / 2 rows), k = size,
# k = size - 1 (two windows), clamping (k > size), odd sizes, two channel vectors per pixel and more than one 256-thread block
BOX_CASES = [((1, 8, 9, 11), (4, 6)), ((2, 8, 12, 20), (5, 5)), ((1, 8, 8, 16), (8, 3)), ((1, 8, 6, 10), (1, 1)), ((2, 16, 37, 45), (6, 9)),
             ((1, 24, 40, 33), (17, 2)), ((1, 8, 21, 64), (20, 40)), ((1, 8, 5, 7), (9, 9)), ((3, 64, 19, 23), (2, 23))]


@pytest.mark.parametrize("shape,k", BOX_CASES)
def test_box_mean_index_arithmetic(dev, shape, k):
    from dcpt_amd import functional as DF
    from kernel_trace import kernel_trace
    from redzone import redzone

    x = keyed_input(f"tlscbf.box.{shape}.{k}", shape, lo=-2.0, hi=3.0).bfloat16()
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    with kernel_trace() as tr, redzone() as rz:
        y = DF.box_mean_bf16(xd, *k)
    tr.assert_ran("tlsc.box_mean_bf16")
    assert rz.count == 2 and y.dtype == torch.bfloat16
    k1, k2 = min(k[0], shape[2]), min(k[1], shape[3])
    ref = _box_mean_f64(x.float(), k1, k2)
    d = (y.float().cpu().double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + k1 * k2 * 2.0 ** -24 * float(x.float().abs().mean())
    worst = float((d - bound).max())
    print(f"{shape} k={k}: max |d| {float(d.max()):.3e}, max (|d| - bound) {worst:.3e}")
    assert bool((d <= bound).all()), (shape, k, float(d.max()), worst)
    if k == (1, 1):
        assert torch.equal(y.cpu(), x)
