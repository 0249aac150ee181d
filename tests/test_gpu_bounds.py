"""Do the entry points stay inside the buffers they are given?  Every workspace-taking family of dcpt_amd/functional.py runs forward and
backward under the red zone (tests/redzone.py: exact-size workspaces and outputs with a guard behind each) at shapes whose last GEMM tile
is partly empty, and is compared with the torch restatement its own test module already holds, at that module's tolerances.  Then the
bf16 bottleneck node at the ragged tails of its 256-row kernel: parity, a white-box check of the workspace bytes a correct library never
writes, the geometry the one-call entry points assume, and the LayerNorm biases its backward reads."""

import pytest
import torch
import torch.nn.functional as F

from dcpt_amd.keyed_init import keyed_input, keyed_tensor
from kernel_trace import kernel_trace
from oracle import dc_oracle as D
from redzone import PATTERN, redzone
from tests import test_gpu_bf16 as TBF
from tests import test_gpu_dchead as TDC
from tests import test_gpu_parity as TPA
from tests import test_gpu_promptir as TPR
from tests import test_gpu_rcan as TRC
from tests import test_gpu_restormer as TRS
from tests import test_gpu_swinir as TSW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dcpt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def guarded(fn, *args):
    with redzone() as rz:
        fn(*args)
    assert rz.count > 0, "nothing was allocated through the patched helpers: the red zone checked nothing"


# ---- the sweep: M = B H W at the edges of the 128-, 256- and 512-row tiles -----------------------------------------------------------
# (M % 128 == 1: one row in the last tile; M % 256 == 128: the 256-row tile's second half starts at M; M % 256 == 129: one row in it)
@pytest.mark.parametrize("B,c,H,W", [(1, 32, 3, 43), (3, 64, 8, 16), (1, 256, 5, 77), (1, 512, 9, 57), (2, 128, 13, 11)])
def test_nafblock_fp32(dev, B, c, H, W):
    guarded(TPA.test_nafblock_oracle, dev, B, c, H, W)


@pytest.mark.parametrize("shape", [(1, 64, 3, 43), (3, 128, 8, 16), (1, 256, 5, 77), (1, 512, 9, 57),
                                   # the 256-row kernel (>= 192 tiles of 256 at C = 256): M % 256 == 1; and M % 256 == 128 with whole
                                   # 128-pixel images, where SCA's channel sums come out of the EB_DOTCOL epilogue
                                   (1, 256, 77, 645), (1, 256, 128, 385),
                                   # the wide levels' chain kernels with a ragged last tile (M = 13 * 1537 = 19981, M % 128 == 13)
                                   (13, 512, 29, 53)])
def test_nafblock_bf16(dev, shape):
    with kernel_trace() as tr:
        guarded(TBF.test_nafblock_bf16_oracle, dev, shape)
    B, c, H, W = shape
    if c == 256 and B * H * W >= 192 * 256:
        tr.assert_ran("nt_bf16.256")


@pytest.mark.parametrize("B,Cin,Cout,H,W,ks,relu,res", [(1, 16, 32, 3, 43, 1, True, False), (3, 64, 64, 8, 16, 3, True, True),
                                                         (1, 128, 256, 5, 77, 1, False, True), (1, 256, 128, 9, 57, 3, True, False)])
def test_conv_ln_fp32(dev, B, Cin, Cout, H, W, ks, relu, res):
    guarded(TDC.test_conv_ln, dev, B, Cin, Cout, H, W, ks, relu, res)


@pytest.mark.parametrize("B,Cin,Cout,H,W,ks,use_res,relu", [(1, 16, 32, 3, 43, 1, False, True), (3, 64, 64, 8, 16, 3, True, True),
                                                             (1, 128, 256, 77, 645, 1, True, True), (1, 128, 256, 128, 385, 3, False, True),
                                                             # the 512 x 128 tile: M % 512 == 1 (1 x 1) and M % 512 == 129 (3 x 3)
                                                             (1, 64, 128, 71, 1399, 1, True, True), (1, 128, 128, 257, 385, 3, False, True)])
def test_conv_ln_bf16(dev, B, Cin, Cout, H, W, ks, use_res, relu):
    guarded(TBF.test_conv_ln_bf16_oracle, dev, B, Cin, Cout, H, W, ks, use_res, relu)


@pytest.mark.parametrize("B,C,H,W,bf", [(1, 16, 3, 43, False), (3, 64, 8, 16, False), (1, 16, 3, 43, True), (3, 64, 8, 16, True),
                                        (1, 128, 5, 77, True), (2, 64, 15, 13, True)])
def test_bottleneck(dev, B, C, H, W, bf):
    guarded(TDC.test_bottleneck_node, dev, B, C, H, W, bf)


@pytest.mark.parametrize("B,C,H,W", [(1, 16, 6, 86), (3, 64, 16, 16), (1, 256, 10, 78)])
def test_down_up(dev, B, C, H, W):
    guarded(TPA.test_down_up, dev, B, C, H, W)
    guarded(TBF.test_down_up_bf16_oracle, dev, B, C, H, W)


@pytest.mark.parametrize("B,Cs,Cb,H,W", [(1, 3, 16, 3, 43), (3, 3, 64, 8, 16), (1, 3, 64, 5, 77)])
def test_edge_convs(dev, B, Cs, Cb, H, W):
    guarded(TPA.test_edge_convs, dev, B, Cs, Cb, H, W)
    guarded(TBF.test_edge_convs_bf16_oracle, dev, B, Cs, Cb, H, W)


def test_dc_head(dev, golden_dir):
    guarded(TDC.test_dc_head_golden, dev, golden_dir)
    guarded(TBF.test_dc_head_bf16_oracle, dev)


@pytest.mark.parametrize("lnt,dim,heads,B,H,W", [("WithBias", 48, 2, 1, 3, 43), ("BiasFree", 64, 2, 3, 8, 16), ("WithBias", 32, 1, 1, 5, 77)])
def test_restormer_block(dev, lnt, dim, heads, B, H, W):
    guarded(TRS.test_block_oracle, dev, lnt, dim, heads, B, H, W)


@pytest.mark.parametrize("lnt,dim,heads,B,H,W", [("WithBias", 160, 4, 1, 3, 43), ("BiasFree", 320, 4, 3, 8, 16)])
def test_promptir_block(dev, lnt, dim, heads, B, H, W):
    guarded(TPR.test_block_oracle, dev, lnt, dim, heads, B, H, W)


@pytest.mark.parametrize("C,heads,ws,B,H,W", [(36, 6, 8, 1, 8, 24), (60, 6, 4, 3, 12, 4), (180, 6, 8, 1, 24, 8), (12, 4, 2, 1, 2, 86)])
def test_swinir_block(dev, C, heads, ws, B, H, W):
    """window attention, MLP and their LayerNorms at M = 192 / 144 / 192 / 172 pixels (H, W multiples of the window: SwinIR refuses others)"""
    from basicsr.archs.swinir_arch import SwinTransformerBlock
    from dcpt_amd.keyed_init import fill_module_

    for shift in (0, ws // 2):
        blk = SwinTransformerBlock(C, (128, 128), heads, ws, shift, 2.0)
        fill_module_(blk, seed=C + shift)
        blk = blk.to(dev)
        P = {k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
        x = keyed_input(f"bnd.sw{C}", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
        go = keyed_input(f"bnd.sw{C}.go", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
        xr, xg = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        yr = TSW.ref_block(xr, P, "", heads, ws, shift)
        yr.backward(go)
        with redzone() as rz, kernel_trace() as tr:
            y = blk(xg)
            y.backward(go)
        assert rz.count > 0
        tr.assert_ran("swin_wattn_fwd", "swin_wattn_bwd")
        TSW.check(f"y shift={shift}", y, yr, 5e-5)
        TSW.check(f"dx shift={shift}", xg.grad, xr.grad, 2e-4)
        for k, p in blk.named_parameters():
            TSW.check(f"grad {k} shift={shift}", p.grad, P[k].grad, 3e-4)


def test_swinir_net_conv3x3_res(dev):
    guarded(TSW.test_net_vs_restatement, dev, 1, 24, 40)


@pytest.mark.parametrize("C,sq,B,H,W", [(64, 16, 5, 7, 9), (64, 16, 3, 43, 3), (32, 4, 2, 8, 8), (128, 16, 1, 3, 43), (64, 16, 7, 11, 12)])
def test_rcab(dev, C, sq, B, H, W):
    """images of 63 / 129 / 64 / 129 / 132 pixels: several share a 128-row tile, or one spills one row into the next (E_BIASCOL's
    per-image column sums)"""
    from basicsr.archs.rcan_arch import RCAB
    from dcpt_amd.keyed_init import fill_module_

    blk = RCAB(C, sq, 0.5)
    fill_module_(blk, seed=C + H)
    blk = blk.to(dev)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
    x = keyed_input(f"bnd.rc{C}.{H}", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
    go = keyed_input(f"bnd.rc{C}.{H}.go", (B, C, H, W), lo=-1.0, hi=1.0).to(dev)
    xr, xg = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr = TRC.ref_rcab(xr, P, "", 0.5)
    yr.backward(go)
    with redzone() as rz:
        y = blk(xg)
        y.backward(go)
    assert rz.count > 0
    TRC.check("y", y, yr, 5e-5)
    TRC.check("dx", xg.grad, xr.grad, 2e-4)
    for k, p in blk.named_parameters():
        TRC.check(f"grad {k}", p.grad, P[k].grad, 3e-4)


@pytest.mark.parametrize("s,B,h,w", [(2, 1, 3, 43), (3, 3, 8, 16), (2, 2, 9, 7)])
def test_rcan_net_conv3x3_ps(dev, s, B, h, w):
    guarded(TRC.test_net_vs_restatement, dev, s, B, h, w)


# ---- the bf16 bottleneck at the ragged tails of the 256-row kernel (2C == 256, >= 192 tiles of 256 pixels) ------------------------------
RAGGED = [(1, 257, 513),     # M = 131 841, M % 256 = 1
          (1, 128, 1025),    # M = 131 200, M % 256 = 128: the last tile's second half starts at M
          (32, 125, 125),    # M = 500 000, M % 256 = 32: stage 1 of the DCPT head at B = 32
          (1, 255, 515)]     # M = 131 325, M % 256 = 253 (control: both halves hold rows)


def _bneck_params(C):
    Cb = 2 * C
    return [keyed_tensor("bnr.conv1.weight", (Cb, C, 1, 1)), keyed_tensor("bnr.norm1.weight", (Cb,)), keyed_tensor("bnr.norm1.bias", (Cb,)),
            keyed_tensor("bnr.conv2.weight", (Cb, Cb, 3, 3)), keyed_tensor("bnr.norm2.weight", (Cb,)), keyed_tensor("bnr.norm2.bias", (Cb,)),
            keyed_tensor("bnr.conv3.weight", (C, Cb, 1, 1)), keyed_tensor("bnr.norm3.weight", (C,)), keyed_tensor("bnr.norm3.bias", (C,))]


def _fp64_block(x, ws, go):
    """the reference's lines (degrad_classify_arch.py:227-243) in float64 on the device: y, [dx, dw1, dlw1, ..., dlb3]"""
    ref = [t.double().requires_grad_(True) for t in [x] + ws]
    r = F.relu(D.layernorm_cf(F.conv2d(ref[0], ref[1]), ref[2], ref[3]))
    r = F.relu(D.layernorm_cf(F.conv2d(r, ref[4], padding=1), ref[5], ref[6]))
    r = F.relu(D.layernorm_cf(F.conv2d(r, ref[7]), ref[8], ref[9]) + ref[0])
    r.backward(go.double())
    return r.detach(), [t.grad for t in ref]


def _check_vs_fp64(y, grads, yr, gr):
    # the bf16 tolerances of test_gpu_bf16.test_conv_ln_bf16_oracle against the unrounded chain: ReLU masks of values that round across zero
    # flip whole gradient entries, so these are bounds, not the 2e-2 of a comparison with bf16 roundings restated.  That test bounds dx
    # only without a ReLU: behind three ReLUs a flipped mask moves single elements of dx by a large share of its maximum (0.79 of it in a
    # CPU emulation of this block with bf16 forward storage), so dx is held to its relative L2 error instead: 6.4-6.9e-2 measured on
    # MI355X for the node and for the chain alike (the two agree within the 2e-2 above), a tile of wrong or missing rows is far beyond 0.1
    TDC.check("y vs fp64", y.float(), yr, 4e-2)
    dx, dxr = grads[0].double(), gr[0]
    e = float((dx - dxr).norm() / dxr.norm())
    assert e <= 0.1, f"dx vs fp64: relative L2 error {e:.3e} > 0.1"
    for n, a, b in zip(["dw1", "dlw1", "dlb1", "dw2", "dlw2", "dlb2", "dw3", "dlw3", "dlb3"], grads[1:], gr[1:]):
        TDC.check(n + " vs fp64", a.float(), b, 0.15)


@pytest.mark.parametrize("B,H,W", RAGGED)
def test_bottleneck_bf16_ragged_256_tail(dev, B, H, W):
    from dcpt_amd import functional as DF

    C = 128
    ws = _bneck_params(C)
    x = keyed_input("bnr.x", (B, C, H, W), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    go = keyed_input("bnr.go", (B, C, H, W), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)

    def node(packed):
        xg = x.detach().clone().requires_grad_(True)
        pg = [t.to(dev).requires_grad_(True) for t in ws]
        packs = (DF.PackedConvBf16(), DF.PackedConvBf16(), DF.PackedConvBf16()) if packed else None
        with redzone() as rz, kernel_trace() as tr:
            y = DF.bottleneck(xg, *pg, packs=packs)
            y.backward(go)
        assert rz.count > 0
        tr.assert_ran("head.conv1x1_dgrad+ln_bwd_epilogue", "head.conv3x3_dgrad+ln_bwd_epilogue", "nt_bf16.256", "nt_bf16.256_conv3")
        tr.assert_ran("head.wpack_multi" if packed else "head.wpack_per_call")
        return y.detach(), [xg.grad] + [p.grad for p in pg]

    y, grads = node(False)
    y_pk, grads_pk = node(True)
    # the cached images and the per-call packs are the same bytes: any difference is a write into the operand the GEMM reads
    assert torch.equal(y, y_pk)
    for n, a, b in zip(["dx", "dw1", "dlw1", "dlb1", "dw2", "dlw2", "dlb2", "dw3", "dlw3", "dlb3"], grads, grads_pk):
        assert torch.equal(a, b), f"{n}: cached packs vs packs per call (max diff {float((a - b).abs().max()):.3e})"
    # the three-node chain, with the assertions of test_gpu_dchead.test_bottleneck_node
    xc = x.detach().clone().requires_grad_(True)
    pc = [t.to(dev).requires_grad_(True) for t in ws]
    o = DF.conv_ln_bf16(xc, pc[0], pc[1], pc[2], None, True)
    o = DF.conv_ln_bf16(o, pc[3], pc[4], pc[5], None, True)
    yc = DF.conv_ln_bf16(o, pc[6], pc[7], pc[8], xc, True)
    yc.backward(go)
    assert torch.equal(y, yc), "the forward of the node is the three calls of the chain"
    TDC.check("dx vs chain", grads[0].float(), xc.grad.float(), 2e-2)
    for n, a, b in zip(["dw1", "dlw1", "dlb1", "dw2", "dlw2", "dlb2", "dw3", "dlw3", "dlb3"], grads[1:], pc):
        if n in ("dw1", "dlw1", "dlb1", "dw2", "dlw2", "dlb2"):
            TDC.check(n, a, b.grad, 1e-3)
        else:
            assert torch.equal(a, b.grad), f"{n}: max diff {float((a - b.grad).abs().max()):.3e}"
    del xc, pc, o, yc
    yr, gr = _fp64_block(x.float(), [t.to(dev) for t in ws], go.float())
    _check_vs_fp64(y, grads, yr, gr)


def _align(n, a=256):
    return (n + a - 1) // a * a


@pytest.mark.parametrize("B,H,W", RAGGED[:3])
def test_bottleneck_bf16_bwd_writes_no_packed_weight_region(dev, B, H, W):
    """White box: dcpt_bottleneck_bwd_bf16 with cached packs never writes the per-call weight images cw[1].wp / cw[2].wp of its workspace.
    The workspace is allocated here and filled with the pattern; afterwards those regions must still hold it.  A column-sum row stored
    past cw[k - 1].lnpart (the last 128-row half of a ragged 256-row tile) lands exactly there."""
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    lib = _lib.load()
    C = 128
    Cb = 2 * C
    M = B * H * W
    ws = [t.to(dev) for t in _bneck_params(C)]
    x = keyed_input("bnr.x", (B, C, H, W), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    go = keyed_input("bnr.go", (B, C, H, W), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    geo = [(C, Cb, 1), (Cb, Cb, 3), (Cb, C, 1)]   # (Cin, Cout, ks) of the three groups
    packs = [DF.PackedConvBf16() for _ in range(3)]
    DF.pack_convs_bf16([(pk, ws[3 * k]) for k, pk in enumerate(packs)])
    s = DF._stream(dev)
    groups = []
    for k, (Cin, Cout, ks) in enumerate(geo):
        groups.append(dict(z=torch.empty((M, Cout), dtype=torch.bfloat16, device=dev), y=torch.empty((M, Cout), dtype=torch.bfloat16, device=dev),
                           stats=torch.empty((2, M), dtype=torch.float32, device=dev), dw=torch.empty_like(ws[3 * k]),
                           dlw=torch.empty_like(ws[3 * k + 1]), dlb=torch.empty_like(ws[3 * k + 1])))

    def garr(backward):
        a = (_lib.BneckGroup * 3)()
        for k, g in enumerate(groups):
            pk = packs[k].buf
            a[k] = _lib.BneckGroup(ws[3 * k].data_ptr(), pk.data_ptr(), pk.numel(), ws[3 * k + 1].data_ptr(), ws[3 * k + 2].data_ptr(),
                                   g["z"].data_ptr(), g["y"].data_ptr(), g["stats"][0].data_ptr(), g["stats"][1].data_ptr(),
                                   g["dw"].data_ptr() if backward else None, g["dlw"].data_ptr() if backward else None,
                                   g["dlb"].data_ptr() if backward else None)
        return a

    nf = lib.dcpt_bottleneck_bf16_ws_bytes(B, H, W, C, 0)
    wsf = torch.empty(nf, dtype=torch.uint8, device=dev)
    _lib.check(lib.dcpt_bottleneck_fwd_bf16(x.data_ptr(), garr(False), wsf.data_ptr(), nf, B, H, W, C, s), "dcpt_bottleneck_fwd_bf16")
    del wsf
    # This mirrors bneck_layout (dcpt_amd/csrc/dchead_bf16.hip) and must follow it: cw[k] starts at the sum of the 256-aligned conv
    # workspaces of the groups before it, and its first allocation is wp, the [Cout][ks ks Cin] bf16 weight image (256-aligned).
    nb = lib.dcpt_bottleneck_bf16_ws_bytes(B, H, W, C, 1)
    start = [0]
    for Cin, Cout, ks in geo:
        start.append(start[-1] + _align(lib.dcpt_conv_ln_bf16_ws_bytes(B, H, W, Cin, Cout, ks, 1)))
    assert start[3] <= nb
    wp_end = [start[k] + _align(geo[k][1] * geo[k][2] ** 2 * geo[k][0] * 2) for k in range(3)]
    wsb = torch.full((nb,), PATTERN, dtype=torch.uint8, device=dev)
    dx = torch.empty((M, C), dtype=torch.bfloat16, device=dev)
    with kernel_trace() as tr:
        _lib.check(lib.dcpt_bottleneck_bwd_bf16(go.data_ptr(), x.data_ptr(), garr(True), dx.data_ptr(), wsb.data_ptr(), nb, B, H, W, C, s),
                   "dcpt_bottleneck_bwd_bf16")
        torch.cuda.synchronize()
    tr.assert_ran("head.conv1x1_dgrad+ln_bwd_epilogue", "head.conv3x3_dgrad+ln_bwd_epilogue")
    tr.assert_not_ran("head.wpack_per_call")
    for k in (1, 2):   # from the end of cw[k - 1] to the end of cw[k].wp
        region = wsb[start[k]: wp_end[k]]
        bad = region != PATTERN
        assert not bool(bad.any()), (f"bytes {start[k]}..{wp_end[k]} (the end of cw[{k - 1}] to the end of cw[{k}].wp) were written: "
                                     f"{int(bad.sum())} bytes, the first at +{int(torch.nonzero(bad)[0])}")
    assert bool(torch.isfinite(dx.float()).all())


# ---- geometry: BottleneckBlock accepts any bottleneck width; only C -> 2C -> 2C -> C takes the one-call entry points ---------------------
@pytest.mark.parametrize("Cb", [96, 64])
def test_bottleneck_bf16_other_widths(dev, Cb):
    from basicsr.archs.degrad_classify_arch import BottleneckBlock
    from dcpt_amd import functional as DF

    C, B, H, W = 64, 2, 9, 11
    blk = BottleneckBlock(C, C, bottleneck_channels=Cb)
    names = ["conv1.weight", "conv1.norm.weight", "conv1.norm.bias", "conv2.weight", "conv2.norm.weight", "conv2.norm.bias",
             "conv3.weight", "conv3.norm.weight", "conv3.norm.bias"]
    sd = {k: keyed_tensor(f"bnw{Cb}." + k, tuple(v.shape)) for k, v in blk.state_dict().items()}
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev)
    ws = [sd[n] for n in names]
    x = keyed_input(f"bnw{Cb}.x", (B, C, H, W), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    go = keyed_input(f"bnw{Cb}.go", (B, C, H, W), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    xg = x.detach().clone().requires_grad_(True)
    with redzone() as rz, kernel_trace() as tr:
        y = blk(xg)
        y.backward(go)
    assert rz.count > 0
    tr.assert_not_ran("head.conv1x1_dgrad+ln_bwd_epilogue", "head.conv3x3_dgrad+ln_bwd_epilogue")   # (the one-call backward's marks)
    grads = [xg.grad] + [dict(blk.named_parameters())[n].grad for n in names]
    xc = x.detach().clone().requires_grad_(True)
    pc = [t.to(dev).requires_grad_(True) for t in ws]
    o = DF.conv_ln_bf16(xc, pc[0], pc[1], pc[2], None, True)
    o = DF.conv_ln_bf16(o, pc[3], pc[4], pc[5], None, True)
    yc = DF.conv_ln_bf16(o, pc[6], pc[7], pc[8], xc, True)
    yc.backward(go)
    assert torch.equal(y, yc)
    TDC.check("dx vs chain", grads[0].float(), xc.grad.float(), 2e-2)
    for n, a, b in zip(names, grads[1:], pc):
        TDC.check(n + " vs chain", a, b.grad, 1e-3)
    yr, gr = _fp64_block(x.float(), [t.to(dev) for t in ws], go.float())
    _check_vs_fp64(y, grads, yr, gr)


# ---- the LayerNorm biases the backward recomputes the ReLU masks with are saved tensors -------------------------------------------------
@pytest.mark.parametrize("how", ["in_place", "fused_adamw"])
def test_bottleneck_bf16_bias_update_before_backward_raises(dev, how):
    from basicsr.archs.degrad_classify_arch import BottleneckBlock
    from dcpt_amd.optim import FusedAdamW

    blk = BottleneckBlock(16, 16, bottleneck_channels=32).to(dev)
    x = keyed_input("bnv.x", (2, 16, 6, 10), lo=-1, hi=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    with kernel_trace() as tr:
        y = blk(x.requires_grad_(True))
    tr.assert_ran("head.conv1x1+ln_fwd_epilogue")
    if how == "in_place":
        with torch.no_grad():
            blk.conv2.norm.bias.add_(0.5)
    else:
        for p in blk.parameters():
            p.grad = torch.ones_like(p)
        FusedAdamW(blk.parameters(), lr=1e-2).step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(torch.ones_like(y))
