"""torch.autograd bindings over the C ABI (include/dcpt_hip.h).

PyTorch is plumbing here: it owns device memory (activations, saved tensors, workspaces), the
stream, and autograd's graph.  All arithmetic happens in libdcpt_hip.so.

Layout: feature maps are ordinary torch tensors of logical shape (N, C, H, W) in
``torch.channels_last`` memory (= NHWC), so forward hooks, DDP and user code see the reference's
shapes while the kernels see contiguous channel rows.  The 3-channel image stays NCHW-contiguous.
"""
from __future__ import annotations

import ctypes as C
import math
import os as _os
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from . import _lib
from ._lib import NafBlockGrads, NafBlockParams, NafBlockSaved, PARAM_FIELDS, check

CL = torch.channels_last
_ws_cache: Dict[Tuple[int, int], torch.Tensor] = {}


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream); kernels using it are stream-ordered."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), _stream(dev))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _ws_cache[key] = buf
    return buf


def release_workspaces():
    _ws_cache.clear()


_NO_CPU = "dcpt_amd kernels run on a HIP device only (got a CPU tensor); there is no CPU fallback"


def _require(ts, dtypes, what, none_ok=True):
    """every tensor of ``ts`` on the device and of one of ``dtypes`` (``what``: the message for another dtype)"""
    for t in ts:
        if t is None and none_ok:
            continue
        if not t.is_cuda:
            raise _lib.DcptHipError(_NO_CPU)
        if t.dtype not in dtypes:
            raise _lib.DcptHipError(what.format(t.dtype))


def _require_gpu(*ts):
    _require(ts, (torch.float32,), "dcpt_amd kernels are fp32 (got {})")


def _require_gpu_feat(*ts):
    """feature maps of the ops that exist in both storage types: fp32 or bf16, on the device"""
    _require(ts, (torch.float32, torch.bfloat16), "feature maps are fp32 or bf16 (got {})")


def _require_gpu_bf16(*ts):
    _require(ts, (torch.bfloat16,), "the bf16-storage path takes torch.bfloat16 activations (got {})", none_ok=False)


# An incoming gradient of an op in bf16 storage that is not bf16 itself: the two policies (DESIGN.md section 4 lists which op has which)
def _grad_strict(dy, bf):
    """strict: a gradient in another dtype than the bf16 storage is an error"""
    if bf:
        _require_gpu_bf16(dy)
    return dy


def _grad_cast(dy, dtype):
    """cast: the gradient is brought to the op's storage dtype"""
    return dy if dy.dtype == dtype else dy.to(dtype)


def _nhwc(x: torch.Tensor) -> torch.Tensor:
    """(N,C,H,W) tensor whose memory is dense NHWC."""
    if x.dim() != 4:
        raise ValueError(f"expected a 4-D NCHW tensor, got {tuple(x.shape)}")
    n, c, h, w = x.shape
    if x.stride() == (h * w * c, 1, w * c, c):
        return x
    return x.contiguous(memory_format=CL) if (c > 1 and h * w > 1) else _force_nhwc(x)


def _force_nhwc(x):
    n, c, h, w = x.shape
    out = torch.empty_strided((n, c, h, w), (h * w * c, 1, w * c, c), dtype=x.dtype, device=x.device)
    out.copy_(x)
    return out


def _empty_nhwc(n, c, h, w, dev) -> torch.Tensor:
    return torch.empty_strided((n, c, h, w), (h * w * c, 1, w * c, c), dtype=torch.float32, device=dev)


def _empty_nhwc_bf16(n, c, h, w, dev) -> torch.Tensor:
    """bf16-storage path (BASELINE.json configs[2]): activations / saved tensors torch.bfloat16 (channels_last), parameters fp32"""
    return torch.empty_strided((n, c, h, w), (h * w * c, 1, w * c, c), dtype=torch.bfloat16, device=dev)


def _empty(bf):
    """the feature-map allocator of a storage type.  _workspace, _empty_nhwc and _empty_nhwc_bf16 are the three names tests/redzone.py
    swaps on this module: they are looked up when called, and the op's own frame calls what this returns."""
    return _empty_nhwc_bf16 if bf else _empty_nhwc


def _p(t):
    return 0 if t is None else t.data_ptr()


def _struct(cls, ts):
    """a *Params / grads struct of the ABI over tensors (None: a NULL field)"""
    return cls(*[_p(t) for t in ts])


def _call(fn, ptrs, dims, dev, ws_bytes=None):
    """The one argument convention of the C ABI (include/dcpt_hip.h): pointers, [workspace, workspace bytes,] integer / float geometry,
    stream.  Of ``ptrs`` a tensor becomes its address, None a null pointer and a ctypes struct a reference; integers and ctypes arrays
    pass through.  ``ws_bytes``: the workspace is requested here, through the module's ``_workspace``."""
    args = []
    for a in ptrs:
        if isinstance(a, torch.Tensor):
            args.append(a.data_ptr())
        elif isinstance(a, C.Structure):
            args.append(C.byref(a))
        else:
            args.append(a)
    if ws_bytes is not None:
        ws = _workspace(dev, ws_bytes)
        args += (ws.data_ptr(), ws.numel())
    check(fn(*args, *dims, _stream(dev)), fn.__name__)


def _contig(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------
# Opt-in GEMM precision mode (include/dcpt_hip.h dcpt_set_gemm_x3): "fp32" = the exact fp32 MFMA kernels (default, the reference's
# arithmetic); "bf16x3" = the wide fp32 GEMMs on the bf16 matrix pipe with operands split into three bf16 pieces (fp32-class results).
# The library's switch is process-wide; here it is driven per NETWORK (``network_g.gemm_precision`` in the options): a network's forward
# runs inside ``gemm_precision(mode)``, every autograd node built there remembers the mode and its backward runs under it again.
_X3_SCRATCH: Dict[int, torch.Tensor] = {}       # device index -> scratch for the split weight images
_GEMM_DEFAULT = ("fp32", 0)                     # the process default: (mode, min_tiles)
_GEMM_ACTIVE = ("fp32", 0)                      # what the library is switched to right now
_GEMM_ACTIVE_BUF = (None, 0)                    # (device index, bytes) of the scratch registered with the library while bf16x3 is on
_GEMM_SCRATCH_MB = 256
_SIDE_BEFORE_X3 = None                          # the side-stream setting the mode found when it was switched on


def _activate_gemm_mode(mode: str, min_tiles: int = 0, device=None):
    global _GEMM_ACTIVE, _GEMM_ACTIVE_BUF, _SIDE_BEFORE_X3
    if (mode, min_tiles) == _GEMM_ACTIVE:
        if mode == "fp32":
            return
        # already on: still re-register when the scratch has to grow (a later set_gemm_precision(scratch_mb=...)) or to move to
        # another device -- otherwise large launches would silently fall back to the fp32 kernels (round-4 advisor finding)
        want = torch.device(device).index if device is not None else _GEMM_ACTIVE_BUF[0]
        if want is None:
            want = torch.cuda.current_device()
        if want == _GEMM_ACTIVE_BUF[0] and _GEMM_ACTIVE_BUF[1] >= (_GEMM_SCRATCH_MB << 20):
            return
    lib = _lib.load()
    if mode == "fp32":
        check(lib.dcpt_set_gemm_x3(None, 0, 0), "dcpt_set_gemm_x3")
        if _SIDE_BEFORE_X3 is not None:
            lib.dcpt_set_side_stream(_SIDE_BEFORE_X3)   # what the caller had, not a hard-wired "on"
            _SIDE_BEFORE_X3 = None
    elif mode == "bf16x3":
        idx = torch.device(device).index if device is not None else torch.cuda.current_device()   # (one process per GPU: its own device)
        if idx is None:
            idx = torch.cuda.current_device()
        buf = _X3_SCRATCH.get(idx)
        if buf is None or buf.numel() < (_GEMM_SCRATCH_MB << 20):
            buf = _X3_SCRATCH[idx] = torch.empty(_GEMM_SCRATCH_MB << 20, dtype=torch.uint8, device=torch.device("cuda", idx))
        check(lib.dcpt_set_gemm_x3(buf.data_ptr(), buf.numel(), int(min_tiles)), "dcpt_set_gemm_x3")
        _GEMM_ACTIVE_BUF = (idx, buf.numel())
        # the split-operand kernels take the whole CU (160 KB of LDS, 8 waves): a weight-gradient block of the side stream cannot share a
        # CU with them (measured: 107.0 ms serialized vs 109.2 ms with it), so the side stream is off while the mode is on
        prev = lib.dcpt_set_side_stream(0)
        if _SIDE_BEFORE_X3 is None:
            _SIDE_BEFORE_X3 = prev
    else:
        raise ValueError(f"gemm precision {mode!r}: expected 'fp32' or 'bf16x3'")
    _GEMM_ACTIVE = (mode, min_tiles)


def set_gemm_precision(mode: str, device=None, scratch_mb: int = 256, min_tiles: int = 0) -> str:
    """Process default: 'fp32' (exact fp32 MFMA, the reference's arithmetic) or 'bf16x3'; returns the previous default.  ``scratch_mb``:
    room for the split images of one launch's weights (6 bytes per element; the per-image conv3 weights of a batch are the largest:
    B x C x C x 6) -- ``gemm_x3_scratch_misses()`` counts eligible launches that did not fit.  ``min_tiles`` > 0 lowers the size
    threshold (tests force the mode onto small launches with 1)."""
    global _GEMM_DEFAULT, _GEMM_SCRATCH_MB
    if mode not in ("fp32", "bf16x3"):
        raise ValueError(f"gemm precision {mode!r}: expected 'fp32' or 'bf16x3'")
    prev = _GEMM_DEFAULT[0]
    _GEMM_SCRATCH_MB = max(_GEMM_SCRATCH_MB, int(scratch_mb))
    _GEMM_DEFAULT = (mode, int(min_tiles))
    _activate_gemm_mode(mode, int(min_tiles), device)
    return prev


def get_gemm_precision() -> str:
    return _GEMM_ACTIVE[0]


def gemm_x3_scratch_misses() -> int:
    return int(_lib.load().dcpt_gemm_x3_scratch_misses())


class gemm_precision:
    """``with gemm_precision(mode):`` -- the GEMM precision for the kernels launched inside (None: leave it as it is); the autograd nodes
    created inside run their backward under the same mode."""

    def __init__(self, mode, min_tiles=None):
        self.want = None if mode is None else (mode, _GEMM_DEFAULT[1] if min_tiles is None else int(min_tiles))

    def __enter__(self):
        self.prev = _GEMM_ACTIVE
        if self.want is not None:
            _activate_gemm_mode(*self.want)
        return self

    def __exit__(self, *exc):
        if self.want is not None:
            _activate_gemm_mode(*self.prev)
        return False


def _remember_gemm_mode(cls, fp32_only=False):
    """forward notes the active mode on the node, backward re-activates it (a no-op comparison when nothing changed).  ``fp32_only``: a
    node whose feature map (its first argument) is in bf16 storage notes nothing, so its backward never switches the mode (a switch also
    turns the side stream off): the mode is an fp32-storage matter, and the bf16-storage forms of these ops have
    always run their backward under whatever was active."""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *args):
        if not (fp32_only and args[0].dtype == torch.bfloat16):
            ctx._gemm_mode = _GEMM_ACTIVE
        return fwd(ctx, *args)

    def backward(ctx, *grads):
        mode = getattr(ctx, "_gemm_mode", _GEMM_ACTIVE)
        if mode == _GEMM_ACTIVE:
            return bwd(ctx, *grads)
        prev = _GEMM_ACTIVE
        _activate_gemm_mode(*mode)
        try:
            return bwd(ctx, *grads)
        finally:
            _activate_gemm_mode(*prev)

    cls.forward = staticmethod(forward)
    cls.backward = staticmethod(backward)
    return cls


def _remember_gemm_mode_fp32(cls):
    return _remember_gemm_mode(cls, fp32_only=True)


# ------------------------------------------------------------------------------------------------
def _saved_f32(t1, t2, y, v, stats, pooled, s, xn):
    """dcpt_nafblock_saved over the forward's buffers; v / stats / xn are None where the library does not use them (NULL pointers)."""
    st = [0, 0, 0, 0] if stats is None else [stats[i].data_ptr() for i in range(4)]
    xs = [0, 0, 0] if xn is None else [xn[i].data_ptr() for i in range(3)]
    return NafBlockSaved(t1.data_ptr(), t2.data_ptr(), y.data_ptr(), 0 if v is None else v.data_ptr(), st[0], st[1], st[2], st[3],
                         pooled.data_ptr(), s.data_ptr(), xs[0], xs[1], xs[2])


@_remember_gemm_mode
class _NAFBlockFn(torch.autograd.Function):
    """reference basicsr/archs/nafnet_arch.py:165-186 (NAFBlock.forward) -> dcpt_nafblock_fwd/bwd."""

    @staticmethod
    def forward(ctx, inp, grad_mode, *params):
        lib = _lib.load()
        _require_gpu(inp, *params)
        inp = _nhwc(inp)
        ctx.owners = params   # (the Parameter objects: their DDP bucket views, if any, receive the gradients)
        params = tuple(_contig(p.detach()) for p in params)
        B, Cc, H, W = inp.shape
        dev = inp.device
        M = B * H * W
        out = _empty_nhwc(B, Cc, H, W, dev)
        t1 = _empty_nhwc(B, 2 * Cc, H, W, dev)
        t2 = _empty_nhwc(B, Cc, H, W, dev)
        y = _empty_nhwc(B, Cc, H, W, dev)
        # where the forward 1 x 1 chains are fused (dcpt_nafblock_fused_ffn) LN1(inp), LN2(y) and the gate do not exist; with no
        # backward coming, v and the statistics are not written either
        fused = bool(lib.dcpt_nafblock_fused_ffn(Cc))
        # (needs_input_grad follows requires_grad alone -- it stays True under torch.no_grad() --, hence the caller's grad mode)
        infer = fused and not (grad_mode and any(ctx.needs_input_grad))
        _NAFBlockFn.last_infer = infer   # (read by the tests: which form the last forward took)
        v = None if infer else _empty_nhwc(B, 2 * Cc, H, W, dev)
        xn = None if fused else torch.empty((3, B, H, W, Cc), dtype=torch.float32, device=dev)   # LN1(inp), LN2(y), SimpleGate(v)
        stats = None if infer else torch.empty((4, M), dtype=torch.float32, device=dev)
        pooled = torch.empty((B, Cc), dtype=torch.float32, device=dev)
        s = torch.empty((B, Cc), dtype=torch.float32, device=dev)
        sv = _saved_f32(t1, t2, y, v, stats, pooled, s, xn)
        _call(lib.dcpt_nafblock_fwd, (_struct(NafBlockParams, params), inp, out, sv), (B, H, W, Cc), dev,
              lib.dcpt_nafblock_fwd_ws_bytes(B, H, W, Cc))
        if not infer:
            ctx.has_xn = xn is not None
            ctx.save_for_backward(inp, t1, t2, y, v, stats, pooled, s, *(() if xn is None else (xn,)), *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        if ctx.has_xn:
            inp, t1, t2, y, v, stats, pooled, s, xn, *params = ctx.saved_tensors
        else:
            (inp, t1, t2, y, v, stats, pooled, s, *params), xn = ctx.saved_tensors, None
        dout = _nhwc(dout)
        B, Cc, H, W = inp.shape
        dev = inp.device
        grads = _grad_buffers(params, ctx.owners)
        dinp = _empty_nhwc(B, Cc, H, W, dev)
        sv = _saved_f32(t1, t2, y, v, stats, pooled, s, xn)
        _call(lib.dcpt_nafblock_bwd, (_struct(NafBlockParams, params), _struct(NafBlockGrads, grads), inp, sv, dout, dinp), (B, H, W, Cc), dev,
              lib.dcpt_nafblock_bwd_ws_bytes(B, H, W, Cc))
        return (dinp, None, *grads)


def nafblock(inp: torch.Tensor, params: Dict[str, torch.Tensor]) -> torch.Tensor:
    """params: dict with the keys of _lib.PARAM_FIELDS (reference state-dict tensors)."""
    return _NAFBlockFn.apply(inp, torch.is_grad_enabled(), *[params[k] for k in PARAM_FIELDS])


# ------------------------------------------------------------------------------------------------
# bf16-storage path (BASELINE.json configs[2]): activations / saved tensors torch.bfloat16 (channels_last), parameters fp32
def _saved_bf16(t1, v, acts, stats, sca, infer):
    """dcpt_nafblock_saved_bf16 over the forward's buffers.  acts / stats have 5 / 4 rows, or 3 / 2 where the fused second half keeps
    nothing but v (dcpt_nafblock_bf16_fused_ffn): the missing pointers are NULL when no backward follows (``infer``: the library then
    skips v as well) and stand-ins that the fused kernels never touch otherwise (the struct's contract asks for non-null in training)."""
    full = acts.shape[0] == 5
    if infer:
        return _lib.NafBlockSavedBf16(t1.data_ptr(), acts[0].data_ptr(), acts[1].data_ptr(), 0, stats[0].data_ptr(), stats[1].data_ptr(), 0, 0,
                                      sca[0].data_ptr(), sca[1].data_ptr(), acts[2].data_ptr(), 0, 0)
    # (v None: no backward follows at a width whose second half is three kernels -- the bias + gate epilogue then keeps the gate only)
    return _lib.NafBlockSavedBf16(t1.data_ptr(), acts[0].data_ptr(), acts[1].data_ptr(), 0 if v is None else v.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
                                  stats[2 if full else 0].data_ptr(), stats[3 if full else 1].data_ptr(), sca[0].data_ptr(), sca[1].data_ptr(),
                                  acts[2].data_ptr(), acts[3 if full else 2].data_ptr(), acts[4 if full else 2].data_ptr())


class _NAFBlockBf16Fn(torch.autograd.Function):
    """NAFBlock.forward (reference nafnet_arch.py:165-186) with bf16 storage -> dcpt_nafblock_fwd_bf16 / bwd_bf16."""

    @staticmethod
    def forward(ctx, inp, packed, grad_mode, *params):
        lib = _lib.load()
        _require_gpu_bf16(inp)
        _require_gpu(*params)
        inp = _nhwc(inp)
        ctx.owners = params
        params = tuple(_contig(p.detach()) for p in params)
        B, Cc, H, W = inp.shape
        if Cc % 8:
            raise _lib.DcptHipError(f"the bf16-storage path needs channel counts that are multiples of 8 (got {Cc})")
        dev = inp.device
        M = B * H * W
        out = _empty_nhwc_bf16(B, Cc, H, W, dev)
        t1 = _empty_nhwc_bf16(B, 2 * Cc, H, W, dev)
        # no backward coming (torch.no_grad / nothing requires grad) and the block's second half is one kernel at this width: the five
        # tensors only that backward reads (v, LN2(y), SimpleGate(v), LN2's statistics) are neither allocated nor written
        # where the block's second half is one kernel, its backward recomputes LN2(y), the gate and LN2's statistics: never allocated
        # (1: C = 64, ffn_bf16.hip -- never touched; 2: C = 256 / 512, chain_bf16.hip -- written for the backward pass only)
        ffn = int(lib.dcpt_nafblock_bf16_fused_ffn(Cc))
        fused = ffn == 1
        nograd = not (grad_mode and any(ctx.needs_input_grad))
        infer = ffn != 0 and nograd
        _NAFBlockBf16Fn.last_infer = infer
        v = None if nograd else _empty_nhwc_bf16(B, 2 * Cc, H, W, dev)   # (conv4's output is read by the backward only)
        slim = fused or infer
        acts = torch.empty((3 if slim else 5, B, H, W, Cc), dtype=torch.bfloat16, device=dev)   # t2, y, LN1(inp) [, LN2(y), SimpleGate(v)]
        stats = torch.empty((2 if slim else 4, M), dtype=torch.float32, device=dev)
        sca = torch.empty((2, B, Cc), dtype=torch.float32, device=dev)           # pooled, s
        sv = _saved_bf16(t1, v, acts, stats, sca, infer)
        _call(lib.dcpt_nafblock_fwd_bf16, (_struct(NafBlockParams, params), *_pkargs(packed), inp, out, sv), (B, H, W, Cc), dev,
              lib.dcpt_nafblock_fwd_bf16_ws_bytes(B, H, W, Cc))
        ctx.packed = packed   # (a plain byte buffer owned by the module; the backward of THIS forward reads the same pack)
        if not nograd:
            ctx.save_for_backward(inp, t1, v, acts, stats, sca, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        inp, t1, v, acts, stats, sca, *params = ctx.saved_tensors
        dout = _nhwc(_grad_cast(dout, torch.bfloat16))
        B, Cc, H, W = inp.shape
        dev = inp.device
        grads = _grad_buffers(params, ctx.owners)
        dinp = _empty_nhwc_bf16(B, Cc, H, W, dev)
        sv = _saved_bf16(t1, v, acts, stats, sca, False)
        _call(lib.dcpt_nafblock_bwd_bf16, (_struct(NafBlockParams, params), *_pkargs(ctx.packed), _struct(NafBlockGrads, grads), inp, sv, dout,
                                           dinp), (B, H, W, Cc), dev, lib.dcpt_nafblock_bwd_bf16_ws_bytes(B, H, W, Cc))
        return (dinp, None, None, *grads)


# parameters whose values the packed operand copies are made from
_PACK_DEPS = ("conv1_w", "conv2_w", "conv3_w", "conv4_w", "conv5_w", "beta", "gamma")


# Generation counter of "the parameters may have changed".  torch's ``_version`` is NOT enough to detect that: fused / foreach
# optimizers (``AdamW(fused=True)``: aten::_fused_adamw_) and updates through ``p.data`` change a parameter's values without bumping
# the parameter's version counter.  Every optimizer step of the process bumps the generation (a global post-step hook), as do
# ``BaseModel.model_ema`` / ``load_network``; code that writes parameters any other way calls ``invalidate_packed_weights()``.
_PACK_GENERATION = 0


def invalidate_packed_weights() -> int:
    """Mark every cached operand copy of the weights (PackedWeightsBf16) stale; returns the new generation."""
    global _PACK_GENERATION
    _PACK_GENERATION += 1
    return _PACK_GENERATION


def _optimizer_step_post_hook(optimizer, args, kwargs):
    # only an optimizer that owns a parameter some pack was made from makes the packs stale (in the DCPT step optimizer_dc.step() must not
    # make the encoder's blocks repack -- with freeze_encoder it is the only optimizer that ever steps); parameters are tagged when packed
    if any(getattr(p, "_dcpt_packdep", False) for grp in optimizer.param_groups for p in grp["params"]):
        invalidate_packed_weights()
    # DistributedDataParallel with gradient_as_bucket_view: remember the bucket views now sitting in .grad (dcpt_amd/ddp.py)
    first = next((p for grp in optimizer.param_groups for p in grp["params"]), None)
    if first is not None and getattr(first, "_dcpt_ddp", False):
        from .ddp import refresh_views

        refresh_views(p for grp in optimizer.param_groups for p in grp["params"])


def _grad_buffers(saved, owners):
    """Output tensors for a fused block's parameter gradients: a fresh tensor per parameter, or -- where DDP's bucket view of that parameter
    is known and not yet used since the last optimizer step (dcpt_amd/ddp.py) -- an alias of the view, so that the kernels write the
    gradient where the all-reduce will read it."""
    outs = []
    for t, p in zip(saved, owners or (None,) * len(saved)):
        v = getattr(p, "_dcpt_grad_view", None) if p is not None else None
        if (v is not None and p.grad is None and not getattr(p, "_dcpt_view_busy", True) and v.shape == t.shape and v.device == t.device
                and v.dtype == t.dtype):
            p._dcpt_view_busy = True
            _grad_buffers.hits += 1
            outs.append(v.view(v.shape))   # a new tensor object on the bucket's storage: AccumulateGrad adopts it as param.grad
        else:
            outs.append(torch.empty_like(t))
    return outs


_grad_buffers.hits = 0   # (gradients written straight into a DDP bucket view so far: read by the tests and bench.py)


register_optimizer_step_post_hook(_optimizer_step_post_hook)


class PackedWeightsBf16:
    """Per-block cache of the operand copies of a NAFBlock's weights for the bf16 path (dcpt_nafblock_wpack_bf16): refreshed -- one
    launch -- when the parameters may have changed since the last pack, reused otherwise: within a training step the forward, the
    backward and, in the DCPT step, both encoder passes share one pack.  "May have changed" = a new generation (any optimizer step,
    EMA update or checkpoint load of the process, ``invalidate_packed_weights()``), a bumped ``_version`` (ordinary in-place updates:
    ``load_state_dict``, ``.copy_``) or a new address (``.to(device)``)."""

    def __init__(self):
        self.key = None
        self.buf = None
        self.stream = None   # the stream the pack was made on, and the event behind it: another stream waits before it reads the pack
        self.event = None    # (tiled inference runs its tile batches on several streams, basicsr/models/sr_model.py::test_tile)

    def __deepcopy__(self, memo):   # a copied module (EMA network, DDP replica) starts with an empty cache of its own
        return type(self)()

    def __reduce__(self):
        return (type(self), ())

    @staticmethod
    def key_of(params: Dict[str, torch.Tensor]):
        return (_PACK_GENERATION,) + tuple((params[k].data_ptr(), params[k]._version) for k in _PACK_DEPS)

    @staticmethod
    def tag(params: Dict[str, torch.Tensor]):
        """mark the parameters a pack depends on: an optimizer step over any of them invalidates the packs (_optimizer_step_post_hook)"""
        for k in _PACK_DEPS:
            params[k]._dcpt_packdep = True

    def get(self, params: Dict[str, torch.Tensor]) -> torch.Tensor:
        key = self.key_of(params)
        if key == self.key:
            if self.stream != _stream(self.buf.device):
                torch.cuda.current_stream(self.buf.device).wait_event(self.event)
            return self.buf
        if key != self.key:
            lib = _lib.load()
            ps = tuple(_contig(params[k].detach()) for k in PARAM_FIELDS)
            _require_gpu(*ps)
            dev = ps[0].device
            Cc = params["conv3_w"].shape[0]
            nbytes = lib.dcpt_nafblock_wpack_bf16_bytes(Cc)
            if self.buf is None or self.buf.numel() != nbytes or self.buf.device != dev:
                self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _call(lib.dcpt_nafblock_wpack_bf16, (_struct(NafBlockParams, ps), self.buf, self.buf.numel()), (Cc,), dev)
            self.key = key
            self.tag(params)
            self.stream = _stream(dev)
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(dev))
        return self.buf


def pack_blocks_bf16(blocks) -> int:
    """Refresh the weight packs of several NAFBlocks in ceil(n / 8) launches (dcpt_nafblock_wpack_bf16_multi) instead of one per block:
    ``blocks`` = [(PackedWeightsBf16, params dict), ...] of a network, called before its forward; only the stale ones are packed, and
    ``PackedWeightsBf16.get`` then finds them current.  Returns how many were packed."""
    stale = []
    for pk, params in blocks:
        key = pk.key_of(params)
        if key != pk.key:
            stale.append((pk, params, key))
    if len(stale) < 2:
        return 0   # (a single block packs itself in get())
    lib = _lib.load()
    n = len(stale)
    ps_arr = (NafBlockParams * n)()
    bufs, nbytes, widths, keep = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int * n)(), []
    dev = None
    for i, (pk, params, key) in enumerate(stale):
        ps = tuple(_contig(params[k].detach()) for k in PARAM_FIELDS)
        _require_gpu(*ps)
        keep.append(ps)
        dev = ps[0].device
        Cc = params["conv3_w"].shape[0]
        need = lib.dcpt_nafblock_wpack_bf16_bytes(Cc)
        if pk.buf is None or pk.buf.numel() != need or pk.buf.device != dev:
            pk.buf = torch.empty(need, dtype=torch.uint8, device=dev)
        ps_arr[i] = _struct(NafBlockParams, ps)
        bufs[i], nbytes[i], widths[i] = pk.buf.data_ptr(), need, Cc
    _call(lib.dcpt_nafblock_wpack_bf16_multi, (ps_arr, bufs, nbytes, widths), (n,), dev)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    for pk, params, key in stale:
        pk.key, pk.stream, pk.event = key, _stream(dev), ev
        pk.tag(params)
    return n


class PackedConvBf16:
    """Cache of ONE conv's two bf16 operand images (forward, data gradient) for the classifier head's bf16 path (dcpt_conv_wpack_bf16_multi,
    ABI 14): the same staleness rule as PackedWeightsBf16 (generation / ``_version`` / address).  ``pack_convs_bf16`` refreshes a whole head
    in three launches before its forward; without it every conv entry point packs its own image per call (68 launches per DCPT step)."""

    def __init__(self):
        self.key = None
        self.buf = None
        self.stream = None
        self.event = None

    def __deepcopy__(self, memo):
        return type(self)()

    def __reduce__(self):
        return (type(self), ())

    @staticmethod
    def key_of(weight: torch.Tensor):
        return (_PACK_GENERATION, weight.data_ptr(), weight._version, tuple(weight.shape))

    def get(self, weight: torch.Tensor) -> torch.Tensor:
        if self.key_of(weight) != self.key:
            pack_convs_bf16([(self, weight)])
        elif self.stream != _stream(self.buf.device):
            torch.cuda.current_stream(self.buf.device).wait_event(self.event)
        return self.buf


CONV_PACK_CACHE = _os.environ.get("DCPT_CONV_PACK_CACHE", "1") != "0"   # False: the head's conv entry points pack per call again (A/B, the bit-identity test)


def pack_convs_bf16(convs) -> int:
    """Refresh the stale ones of ``convs`` = [(PackedConvBf16, weight [Cout][Cin][k][k] fp32), ...] in one call of dcpt_conv_wpack_bf16_multi;
    returns how many were packed."""
    if not CONV_PACK_CACHE:
        return 0
    stale = [(pk, w, pk.key_of(w)) for pk, w in convs if pk.key_of(w) != pk.key]
    if not stale:
        return 0
    lib = _lib.load()
    n = len(stale)
    ws, bufs, nbytes = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_size_t * n)()
    cin, cout, ksz, keep = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), []
    dev = None
    for i, (pk, w, key) in enumerate(stale):
        w_ = _contig(w.detach())
        _require_gpu(w_)
        keep.append(w_)
        dev = w_.device
        Co, Ci, ks = w_.shape[0], w_.shape[1], w_.shape[2]
        need = lib.dcpt_conv_wpack_bf16_bytes(Ci, Co, ks)
        if pk.buf is None or pk.buf.numel() != need or pk.buf.device != dev:
            pk.buf = torch.empty(need, dtype=torch.uint8, device=dev)
        ws[i], bufs[i], nbytes[i], cin[i], cout[i], ksz[i] = w_.data_ptr(), pk.buf.data_ptr(), need, Ci, Co, ks
    _call(lib.dcpt_conv_wpack_bf16_multi, (ws, bufs, nbytes, cin, cout, ksz), (n,), dev)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    for pk, w, key in stale:
        pk.key, pk.stream, pk.event = key, _stream(dev), ev
        w._dcpt_packdep = True
    return n


def _pk(packed, weight):
    """(pointer, bytes) of a conv's cached operand images -- (None, 0) without a cache: the entry point packs in the call"""
    if packed is None or not CONV_PACK_CACHE:
        return None, 0
    buf = packed.get(weight)
    return buf.data_ptr(), buf.numel()


def _pk_buf(packed, weight):
    """the buffer behind _pk (refreshed if stale), or None without a cache: what a node keeps for the backward of THIS forward, which reads
    the same images"""
    return packed.buf if _pk(packed, weight)[0] is not None else None


def _pkargs(buf):
    """(pointer, bytes) of a _pk_buf result; (0, 0) without one: the entry point packs in the call"""
    return _p(buf), 0 if buf is None else buf.numel()


def nafblock_bf16(inp: torch.Tensor, params: Dict[str, torch.Tensor], packed: PackedWeightsBf16 = None) -> torch.Tensor:
    """bf16 activations in / out, fp32 parameters (dict with the keys of _lib.PARAM_FIELDS); ``packed``: the block's weight-pack cache
    (without it every call packs its own operand copies)."""
    buf = packed.get(params) if packed is not None else None
    return _NAFBlockBf16Fn.apply(inp, buf, torch.is_grad_enabled(), *[params[k] for k in PARAM_FIELDS])


def conv1x1_wgrad_bf16(dy: torch.Tensor, x: torch.Tensor, with_bias: bool = True):
    """Weight (and bias) gradient of a 1 x 1 convolution in bf16 storage (dcpt_conv1x1_wgrad_bf16; the four such products of
    NAFBlock's backward, reference nafnet_arch.py:170-186): dy [M][N], x [M][K] bf16 row-major (or NHWC feature maps) ->
    dW [N][K] fp32 (= dy^T x) and db [N] fp32 (column sums of dy)."""
    lib = _lib.load()
    _require_gpu_bf16(dy, x)
    dy2 = (_nhwc(dy).permute(0, 2, 3, 1) if dy.dim() == 4 else dy).reshape(-1, dy.shape[1] if dy.dim() == 4 else dy.shape[-1])
    x2 = (_nhwc(x).permute(0, 2, 3, 1) if x.dim() == 4 else x).reshape(-1, x.shape[1] if x.dim() == 4 else x.shape[-1])
    dy2, x2 = _contig(dy2), _contig(x2)
    M, N = dy2.shape
    K = x2.shape[1]
    if x2.shape[0] != M:
        raise ValueError(f"conv1x1_wgrad_bf16: {tuple(dy2.shape)} vs {tuple(x2.shape)}")
    dev = dy2.device
    dW = torch.empty((N, K), dtype=torch.float32, device=dev)
    db = torch.empty((N,), dtype=torch.float32, device=dev) if with_bias else None
    nws = lib.dcpt_conv1x1_wgrad_bf16_ws_bytes(M, N, K)
    if nws == 0:
        raise _lib.DcptHipError(f"conv1x1_wgrad_bf16: N={N}, K={K} must be positive multiples of 8")
    _call(lib.dcpt_conv1x1_wgrad_bf16, (dy2, x2, dW, db), (M, N, K), dev, nws)
    return (dW, db) if with_bias else dW


class _CastFn(torch.autograd.Function):
    """edge of the bf16 path: fp32 -> bf16 (RNE) in forward, the bf16 gradient back to fp32 in backward (or the reverse)"""

    @staticmethod
    def forward(ctx, x, to_bf16):
        lib = _lib.load()
        ctx.to_bf16 = bool(to_bf16)
        return _cast(lib, x, ctx.to_bf16)

    @staticmethod
    def backward(ctx, g):
        return _cast(_lib.load(), g, not ctx.to_bf16), None


def _cast(lib, x, to_bf16):
    src, dst = (torch.float32, torch.bfloat16) if to_bf16 else (torch.bfloat16, torch.float32)
    if x.dtype == dst:
        return x
    if not x.is_cuda or x.dtype != src:
        raise _lib.DcptHipError(f"cast: expected a {src} device tensor, got {x.dtype} on {x.device}")
    x = _nhwc(x) if x.dim() == 4 else _contig(x)
    if x.numel() % 8:
        raise _lib.DcptHipError("cast: element count must be a multiple of 8")
    y = torch.empty_like(x, dtype=dst)   # preserves the (dense NHWC) strides
    fn = lib.dcpt_cast_f32_bf16 if to_bf16 else lib.dcpt_cast_bf16_f32
    _call(fn, (x, y), (x.numel(),), x.device)
    return y


def to_bf16(x):
    return x if x.dtype == torch.bfloat16 else _CastFn.apply(x, True)


def to_f32(x):
    return x if x.dtype == torch.float32 else _CastFn.apply(x, False)


def nafblock_local(inp: torch.Tensor, params: Dict[str, torch.Tensor], k1: int, k2: int) -> torch.Tensor:
    """TLSC inference forward (reference nafnet_arch.py:277-288 + arch_util.py:313-455): SCA with a k1 x k2 local mean."""
    if torch.is_grad_enabled() and (inp.requires_grad or any(p.requires_grad for p in params.values())):
        raise NotImplementedError("the TLSC NAFNet variant is inference-only: call it under torch.no_grad()")
    lib = _lib.load()
    ps = [_contig(params[k].detach()) for k in PARAM_FIELDS]
    _require_gpu(inp, *ps)
    inp = _nhwc(inp)
    B, Cc, H, W = inp.shape
    out = _empty_nhwc(B, Cc, H, W, inp.device)
    _call(lib.dcpt_nafblock_local_fwd, (_struct(NafBlockParams, ps), inp, out), (B, H, W, Cc, int(k1), int(k2)), inp.device,
          lib.dcpt_nafblock_local_ws_bytes(B, H, W, Cc, k1, k2))
    return out


def nafblock_local_bf16(inp: torch.Tensor, params: Dict[str, torch.Tensor], k1: int, k2: int, packed: PackedWeightsBf16 = None) -> torch.Tensor:
    """TLSC inference forward in bf16 storage (dcpt_nafblock_local_fwd_bf16; reference nafnet_arch.py:277-288 + arch_util.py:313-455): bf16
    activations in / out, fp32 parameters; ``packed``: the block's weight-pack cache as for ``nafblock_bf16`` (without it the call packs its
    own operand copies).  Inference only, like ``nafblock_local``."""
    if torch.is_grad_enabled() and (inp.requires_grad or any(p.requires_grad for p in params.values())):
        raise NotImplementedError("the TLSC NAFNet variant is inference-only: call it under torch.no_grad()")
    lib = _lib.load()
    ps = [_contig(params[k].detach()) for k in PARAM_FIELDS]
    _require_gpu_bf16(inp)
    _require_gpu(*ps)
    inp = _nhwc(inp)
    B, Cc, H, W = inp.shape
    if Cc % 8:
        raise _lib.DcptHipError(f"the bf16-storage path needs channel counts that are multiples of 8 (got {Cc})")
    buf = packed.get(params) if packed is not None else None
    out = _empty_nhwc_bf16(B, Cc, H, W, inp.device)
    _call(lib.dcpt_nafblock_local_fwd_bf16, (_struct(NafBlockParams, ps), *_pkargs(buf), inp, out), (B, H, W, Cc, int(k1), int(k2)), inp.device,
          lib.dcpt_nafblock_local_fwd_bf16_ws_bytes(B, H, W, Cc, int(k1), int(k2)))
    return out


def box_mean_bf16(x: torch.Tensor, k1: int, k2: int) -> torch.Tensor:
    """k1 x k2 local mean of a bf16 feature map, replicate-padded back to its size (dcpt_box_mean_bf16; reference arch_util.py:378-396):
    the pooling of the TLSC block on its own.  No autograd."""
    lib = _lib.load()
    _require_gpu_bf16(x)
    x = _nhwc(x.detach())
    B, Cc, H, W = x.shape
    if Cc % 8:
        raise _lib.DcptHipError(f"box_mean_bf16 needs a channel count that is a multiple of 8 (got {Cc})")
    out = _empty_nhwc_bf16(B, Cc, H, W, x.device)
    _call(lib.dcpt_box_mean_bf16, (x, out), (B, H, W, Cc, int(k1), int(k2)), x.device, lib.dcpt_box_mean_bf16_ws_bytes(B, H, W, Cc, int(k1), int(k2)))
    return out


# ------------------------------------------------------------------------------------------------
class _TakeBatchFn(torch.autograd.Function):
    """x[lo:hi] along the batch axis as a view; the backward builds the zero-padded gradient WITH THE INPUT'S STRIDES (torch's own
    slice backward allocates it NCHW-contiguous, which costs two layout conversions of the whole feature map per use for NHWC
    tensors: one into the NCHW buffer and one back when the producing block reads it)."""

    @staticmethod
    def forward(ctx, x, lo, hi):
        ctx.meta = (tuple(x.shape), tuple(x.stride()), x.dtype, x.device, int(lo), int(hi))
        return x[lo:hi]

    @staticmethod
    def backward(ctx, g):
        shape, stride, dtype, dev, lo, hi = ctx.meta
        # the input's own strides when they describe a dense, non-overlapping layout (contiguous or channels_last: sorted by
        # stride, the strides telescope over the sizes); anything else (expanded / overlapping views) gets a contiguous gradient.
        # Computed arithmetically -- no throw-away allocation of the feature map's size.
        keep, run = len(shape) == 4, 1
        for st, sz in sorted((st, sz) for st, sz in zip(stride, shape) if sz > 1):
            keep, run = keep and st == run, run * sz
        out = torch.empty_strided(shape, stride, dtype=dtype, device=dev) if keep else torch.empty(shape, dtype=dtype, device=dev)
        if lo > 0:
            out[:lo].zero_()
        if hi < shape[0]:
            out[hi:].zero_()
        out[lo:hi].copy_(g)
        return out, None, None


def _private_grad(g) -> bool:
    """True when the incoming gradient may be mutated in place: a dense tensor that owns its storage and that nothing but the autograd
    engine's input buffer (and this frame) references.  A gradient that the consumer's backward hands to several inputs (torch ``add``),
    a view / expanded gradient (``sum``, slicing) or one kept alive elsewhere shows up as a second owner of the tensor or of its storage
    (probed on torch 2.10: private = tensor use count 2, storage use count 2; ``a + b`` = 3 / 3; ``sum`` = a view).  Anything this
    cannot prove private is cloned by the caller."""
    try:
        if g._base is not None or g.requires_grad or g.grad_fn is not None:
            return False
        if g._use_count() > 2 or torch._C._storage_Use_Count(g.untyped_storage()._cdata) > 2:
            return False
        return torch._prims_common.is_non_overlapping_and_dense(g)
    except (AttributeError, RuntimeError):   # (a torch without the probes: never mutate)
        return False


class _TapSplitFn(torch.autograd.Function):
    """(x, x[lo:hi]) for a feature map with TWO consumers -- the network goes on with x, a tap (the classifier head of the DCPT step,
    reference ...pretrain_model.py:60-68,140-163) takes samples lo..hi-1.  With two separate uses autograd builds the tap's zero-padded
    gradient (a fill + a copy of the feature map's size) and then ADDS the two gradients (three more passes, 18 bf16 `add` launches per
    DCPT step at 256 x 256: 1.4 ms); here the tap's gradient is added INTO rows lo..hi-1 of the main path's gradient, in place: one read
    of the slice and a read-modify-write of the same rows -- when that gradient is provably private (_private_grad: the fresh output of
    the layer above's backward, as in the NAFNet / Restormer graphs); otherwise into a copy of it."""

    @staticmethod
    def forward(ctx, x, lo, hi):
        ctx.meta = (tuple(x.shape), tuple(x.stride()), x.dtype, x.device, int(lo), int(hi))
        return x.view(x.shape), x[lo:hi]

    @staticmethod
    def backward(ctx, g, gs):
        shape, stride, dtype, dev, lo, hi = ctx.meta
        if g is None:
            if gs is None:
                return None, None, None
            return _TakeBatchFn.backward(ctx, gs)
        if gs is not None:
            if g.shape != tuple(shape) or not g.is_floating_point() or not _private_grad(g):
                g = g.clone()
            g[lo:hi].add_(gs.to(g.dtype))
        return g, None, None


def _is_nhwc(x) -> bool:
    n, c, h, w = x.shape
    return x.stride() == (h * w * c, 1, w * c, c)


class _TapSplitStrideFn(torch.autograd.Function):
    """(x, x[lo:hi, :, ::s, ::s]): _TapSplitFn for a tap that is nearest-down-sampled by s on its way into the head (the SwinIR step:
    PromptIR_NoImg_DC(downsample=True), degrad_classify_arch.py:634-637).  The tap is a VIEW -- its strides carry the batch range and the
    grid, ``mix`` reads it in place -- so its gradient arrives compact (hi-lo, C, H/s, W/s) and is added into the grid positions of rows
    lo..hi-1 of the main path's gradient by dcpt_grid_add: no zero fill of a full map, no strided scatter, no full-map add.  In place when
    that gradient is provably private (_private_grad), into a copy otherwise; with no main-path gradient at all, dcpt_grid_scatter writes
    the zero-padded map in one pass."""

    @staticmethod
    def forward(ctx, x, lo, hi, stride):
        s = int(stride)
        _require_gpu(x)
        if x.dim() != 4 or s < 1 or s & (s - 1) or x.shape[2] % s or x.shape[3] % s or x.shape[1] % 4:
            raise ValueError(f"tap_split: stride {s} must be a power of two that divides the map {tuple(x.shape)} (channels a multiple of 4)")
        ctx.meta = (tuple(x.shape), int(lo), int(hi), s)
        return x.view(x.shape), x[lo:hi, :, ::s, ::s]

    @staticmethod
    def backward(ctx, g, gs):
        shape, lo, hi, s = ctx.meta
        if gs is None:
            return g, None, None, None
        lib = _lib.load()
        B, Cc, H, W = shape
        _require_gpu(gs, g)
        gs = _nhwc(gs)
        if g is None:
            g = _empty_nhwc(B, Cc, H, W, gs.device)
            _call(lib.dcpt_grid_scatter, (gs, g), (B, lo, hi, H, W, Cc, s), gs.device)
            return g, None, None, None
        if not _is_nhwc(g) or not _private_grad(g):
            g = _force_nhwc(g)
        _call(lib.dcpt_grid_add, (g, gs), (B, lo, hi, H, W, Cc, s), gs.device)
        return g, None, None, None


def tap_split(x, lo, hi, stride=1):
    """-> (x, x[lo:hi]) with the two gradients merged in place on the way back (one use of x downstream, one tap).  ``stride`` s > 1: the
    tap is x[lo:hi, :, ::s, ::s], a view for ``mix`` to read in place; its compact gradient is merged by dcpt_grid_add (fp32 maps)."""
    if stride == 1:
        return _TapSplitFn.apply(x, lo, hi)
    return _TapSplitStrideFn.apply(x, lo, hi, stride)


def take_batch(x, lo, hi):
    """samples lo..hi-1 of a batch (a view in forward, a stride-preserving zero-padded gradient in backward)"""
    return _TakeBatchFn.apply(x, lo, hi)


# ------------------------------------------------------------------------------------------------
class _LayerNorm2dFn(torch.autograd.Function):
    """reference nafnet_arch.py:25-53 (LayerNormFunction)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        lib = _lib.load()
        _require_gpu(x, weight, bias)
        x = _nhwc(x)
        B, Cc, H, W = x.shape
        M = B * H * W
        y = _empty_nhwc(B, Cc, H, W, x.device)
        stats = torch.empty((2, M), dtype=torch.float32, device=x.device)
        w_, b_ = _contig(weight.detach()), _contig(bias.detach())
        _call(lib.dcpt_ln2d_fwd, (x, w_, b_, y, stats[0], stats[1]), (M, Cc, float(eps)), x.device)
        ctx.save_for_backward(x, stats, w_)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, stats, w_ = ctx.saved_tensors
        dy = _nhwc(dy)
        B, Cc, H, W = x.shape
        M = B * H * W
        dx = _empty_nhwc(B, Cc, H, W, x.device)
        dw = torch.empty_like(w_)
        db = torch.empty_like(w_)
        _call(lib.dcpt_ln2d_bwd, (dy, x, stats[0], stats[1], w_, dx, dw, db), (M, Cc), x.device, lib.dcpt_ln2d_bwd_ws_bytes(M, Cc))
        return dx, dw, db, None


def layernorm2d(x, weight, bias, eps=1e-6):
    return _LayerNorm2dFn.apply(x, weight, bias, eps)


# ------------------------------------------------------------------------------------------------
class _IntroFn(torch.autograd.Function):
    """3x3 conv, image NCHW -> features NHWC (reference nafnet_arch.py:202-210, :252).  The image, the parameters and their gradients are
    fp32; ``out_bf16`` puts the feature side (y, and the dy that comes back) in bf16 storage (edge_bf16.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_bf16):
        lib = _lib.load()
        _require_gpu(x, weight, bias)
        x = _contig(x)
        w_, b_ = _contig(weight.detach()), (None if bias is None else _contig(bias.detach()))
        B, Cin, H, W = x.shape
        Cout = w_.shape[0]
        bf = bool(out_bf16)
        y = _empty(bf)(B, Cout, H, W, x.device)
        _call(lib.dcpt_conv3x3_in_fwd_bf16 if bf else lib.dcpt_conv3x3_in_fwd, (x, w_, b_, y), (B, H, W, Cin, Cout), x.device)
        ctx.save_for_backward(x, w_)
        ctx.has_bias, ctx.bf = bias is not None, bf
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_ = ctx.saved_tensors
        dy = _nhwc(_grad_strict(dy, ctx.bf))
        B, Cin, H, W = x.shape
        Cout = w_.shape[0]
        dev = x.device
        dw = torch.empty_like(w_)
        db = torch.empty((Cout,), dtype=torch.float32, device=dev)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _call(lib.dcpt_conv3x3_in_bwd_bf16 if ctx.bf else lib.dcpt_conv3x3_in_bwd, (dy, x, w_, dx, dw, db), (B, H, W, Cin, Cout), dev,
              lib.dcpt_conv3x3_in_bwd_ws_bytes(B, H, W, Cin, Cout))
        return dx, dw, (db if ctx.has_bias else None), None


class _EndingFn(torch.autograd.Function):
    """3x3 conv, features NHWC -> image NCHW, + residual image (reference nafnet_arch.py:211-219, :271-272).  Features (and dx) fp32 or
    bf16 by x.dtype; the image, the residual image, the parameters and their gradients are fp32 in both."""

    @staticmethod
    def forward(ctx, x, weight, bias, res):
        lib = _lib.load()
        _require_gpu_feat(x)
        _require_gpu(weight, bias, res)
        x = _nhwc(x)
        w_, b_ = _contig(weight.detach()), (None if bias is None else _contig(bias.detach()))
        res_ = None if res is None else _contig(res)
        B, Cin, H, W = x.shape
        Cout = w_.shape[0]
        y = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
        _call(lib.dcpt_conv3x3_out_fwd_bf16 if x.dtype == torch.bfloat16 else lib.dcpt_conv3x3_out_fwd, (x, w_, b_, res_, y),
              (B, H, W, Cin, Cout), x.device)
        ctx.save_for_backward(x, w_)
        ctx.has_bias = bias is not None
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_ = ctx.saved_tensors
        bf = x.dtype == torch.bfloat16
        dy = _contig(dy)
        B, Cin, H, W = x.shape
        Cout = w_.shape[0]
        dev = x.device
        dx = _empty(bf)(B, Cin, H, W, dev)
        dw = torch.empty_like(w_)
        db = torch.empty((Cout,), dtype=torch.float32, device=dev)
        _call(lib.dcpt_conv3x3_out_bwd_bf16 if bf else lib.dcpt_conv3x3_out_bwd, (dy, x, w_, dx, dw, db), (B, H, W, Cin, Cout), dev,
              lib.dcpt_conv3x3_out_bwd_ws_bytes(B, H, W, Cin, Cout))
        return dx, dw, (db if ctx.has_bias else None), (dy if ctx.has_res and ctx.needs_input_grad[3] else None)


def conv3x3_in(x, weight, bias, out_bf16=False):
    """3x3 conv image -> features; ``out_bf16``: emit bf16-storage features (the first layer of the bf16 path)"""
    return _IntroFn.apply(x, weight, bias, out_bf16)


def conv3x3_out(x, weight, bias, res=None):
    return _EndingFn.apply(x, weight, bias, res)


# ------------------------------------------------------------------------------------------------
def _down2x2_ws(lib, bf):
    return lib.dcpt_down2x2_bf16_ws_bytes if bf else lib.dcpt_down2x2_ws_bytes


def _down_fwd(lib, ctx, x, weight, bias):
    """Conv2d(C, 2C, 2, 2) for _DownFn / _DownSkipFn (each has checked x its own way): keeps (x, w_) on ctx, returns y and the NHWC x"""
    _require_gpu(weight, bias)
    x = _nhwc(x)
    bf = x.dtype == torch.bfloat16
    w_, b_ = _contig(weight.detach()), (None if bias is None else _contig(bias.detach()))
    B, Cc, H, W = x.shape
    if H % 2 or W % 2:
        raise ValueError(f"down2x2: H={H}, W={W} must be even")
    y = _empty(bf)(B, 2 * Cc, H // 2, W // 2, x.device)
    _call(lib.dcpt_down2x2_fwd_bf16 if bf else lib.dcpt_down2x2_fwd, (x, w_, b_, y), (B, H, W, Cc), x.device,
          _down2x2_ws(lib, bf)(B, H, W, Cc, 0))
    ctx.save_for_backward(x, w_)
    ctx.has_bias = bias is not None
    return y, x


def _down_bwd(lib, ctx, dy, dx_add):
    """backward of _down_fwd: dx = dx_add + conv^T(dy) (dx_add may be None); dy and dx_add dense NHWC in x's storage"""
    x, w_ = ctx.saved_tensors
    bf = x.dtype == torch.bfloat16
    B, Cc, H, W = x.shape
    dev = x.device
    dx = _empty(bf)(B, Cc, H, W, dev)
    dw = torch.empty_like(w_)
    db = torch.empty((2 * Cc,), dtype=torch.float32, device=dev)
    _call(lib.dcpt_down2x2_bwd_bf16 if bf else lib.dcpt_down2x2_bwd, (dy, x, w_, dx_add, dx, dw, db), (B, H, W, Cc), dev,
          _down2x2_ws(lib, bf)(B, H, W, Cc, 1))
    return dx, dw, (db if ctx.has_bias else None)


# (known, and behaviour: _DownFn notes the gemm mode for fp32 storage only, _DownSkipFn for both storages)
@_remember_gemm_mode_fp32
class _DownFn(torch.autograd.Function):
    """Conv2d(C, 2C, 2, 2) (reference nafnet_arch.py:230); fp32 or bf16 storage (edge_bf16.hip) by x.dtype, parameters fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_gpu_feat(x)
        return _down_fwd(_lib.load(), ctx, x, weight, bias)[0]

    @staticmethod
    def backward(ctx, dy):
        dy = _nhwc(_grad_strict(dy, ctx.saved_tensors[0].dtype == torch.bfloat16))
        return _down_bwd(_lib.load(), ctx, dy, None)


def _up_ps_ws(lib, bf):
    return lib.dcpt_up_ps_bf16_ws_bytes if bf else lib.dcpt_up_ps_ws_bytes


@_remember_gemm_mode_fp32
class _UpFn(torch.autograd.Function):
    """Conv2d(C, 2C, 1, bias=False) + PixelShuffle(2) + skip add (reference nafnet_arch.py:238-242, :264-265); fp32 or bf16 storage
    (edge_bf16.hip) by x.dtype -- the skip is stored like x --, the weight fp32."""

    @staticmethod
    def forward(ctx, x, weight, skip):
        lib = _lib.load()
        _require_gpu_feat(x, skip)
        _require_gpu(weight)
        if skip is not None and skip.dtype != x.dtype:
            raise _lib.DcptHipError("up_ps: x and skip must have the same storage dtype")
        x = _nhwc(x)
        bf = x.dtype == torch.bfloat16
        w_ = _contig(weight.detach())
        skip_ = None if skip is None else _nhwc(skip)
        B, Cc, H, W = x.shape
        y = _empty(bf)(B, Cc // 2, 2 * H, 2 * W, x.device)
        _call(lib.dcpt_up_ps_fwd_bf16 if bf else lib.dcpt_up_ps_fwd, (x, w_, skip_, y), (B, H, W, Cc), x.device, _up_ps_ws(lib, bf)(B, H, W, Cc, 0))
        ctx.save_for_backward(x, w_)
        ctx.has_skip = skip is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_ = ctx.saved_tensors
        bf = x.dtype == torch.bfloat16
        dy = _nhwc(_grad_strict(dy, bf))
        B, Cc, H, W = x.shape
        dev = x.device
        dx = _empty(bf)(B, Cc, H, W, dev)
        dw = torch.empty_like(w_)
        _call(lib.dcpt_up_ps_bwd_bf16 if bf else lib.dcpt_up_ps_bwd, (dy, x, w_, dx, dw), (B, H, W, Cc), dev, _up_ps_ws(lib, bf)(B, H, W, Cc, 1))
        return dx, dw, (dy if ctx.has_skip else None)


def down2x2(x, weight, bias):
    return _DownFn.apply(x, weight, bias)


@_remember_gemm_mode
class _DownSkipFn(torch.autograd.Function):
    """(down2x2(x), x) for an encoder group's output, which has TWO consumers: the down layer and the skip connection into the decoder
    (reference nafnet_arch.py:255-258, :264-265).  As two uses autograd sums the two gradients with a pass of its own over the feature map
    (four `add` launches per step, the level-0 one over the largest tensor of the network); here the skip's gradient -- the up layer's
    dy, untouched -- is the ``dx_add`` of the down layer's backward (dcpt_down2x2_bwd*): summed in the scatter epilogue of
    its data-gradient GEMM.  fp32 or bf16 activations by x.dtype."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        (_require_gpu_bf16 if x.dtype == torch.bfloat16 else _require_gpu)(x)
        y, x = _down_fwd(_lib.load(), ctx, x, weight, bias)
        return y, x.view(x.shape)

    @staticmethod
    def backward(ctx, dy, dskip):
        if dy is None:   # (only the skip was used downstream)
            return dskip, None, None
        if dskip is not None:
            dskip = _nhwc(_grad_cast(dskip, ctx.saved_tensors[0].dtype))
        return _down_bwd(_lib.load(), ctx, _nhwc(dy), dskip)


def down2x2_skip(x, weight, bias):
    """-> (down2x2(x), x): the second output is the skip connection's view of x; the two gradients are summed inside the down layer's
    data-gradient GEMM on the way back"""
    return _DownSkipFn.apply(x, weight, bias)


def up_ps(x, weight, skip=None):
    return _UpFn.apply(x, weight, skip)


# ------------------------------------------------------------------------------------------------
def fused_bias_act(x, bias, ref, act: int, grad: int, alpha: float, scale: float):
    """API parity with the reference's fused_act_ext.fused_bias_act
    (basicsr/ops/fused_act/src/fused_bias_act.cpp:14-26): NCHW input, bias over dim 1."""
    lib = _lib.load()
    _require_gpu(x)
    x = _contig(x)
    y = torch.empty_like(x)
    use_bias = bias is not None and bias.numel() > 0
    use_ref = ref is not None and ref.numel() > 0
    step_b = 1
    for d in x.shape[2:]:
        step_b *= int(d)
    b_ = _contig(bias) if use_bias else None
    r_ = _contig(ref) if use_ref else None
    _call(lib.dcpt_fused_bias_act, (x, b_, r_, y), (x.numel(), x.shape[1] if x.dim() > 1 else 1, step_b, act, grad, float(alpha), float(scale)),
          x.device)
    return y


class _FusedLeakyReLUFn(torch.autograd.Function):
    """reference basicsr/ops/fused_act/fused_act.py:55-82 (first-order part)."""

    @staticmethod
    def forward(ctx, x, bias, negative_slope, scale):
        out = fused_bias_act(x, bias, None, 3, 0, negative_slope, scale)
        ctx.save_for_backward(out)
        ctx.negative_slope, ctx.scale = negative_slope, scale
        return out

    @staticmethod
    def backward(ctx, grad_output):
        (out,) = ctx.saved_tensors
        gi = fused_bias_act(grad_output, None, out, 3, 1, ctx.negative_slope, ctx.scale)
        dims = [0] + list(range(2, gi.dim()))
        return gi, gi.sum(dims), None, None


def fused_leaky_relu(x, bias, negative_slope=0.2, scale=2 ** 0.5):
    return _FusedLeakyReLUFn.apply(x, bias, negative_slope, scale)


# ------------------------------------------------------------------------------------------------
# degradation-classifier head (reference basicsr/archs/degrad_classify_arch.py)
def _conv_ln_ws(lib, bf):
    return lib.dcpt_conv_ln_bf16_ws_bytes if bf else lib.dcpt_conv_ln_ws_bytes


def _conv_ln_fwd(lib, x, w_, pk, lw, lb, res, relu):
    """ONE conv -> channels-first LayerNorm -> [+res] -> [ReLU] group: dcpt_conv_ln_fwd, or dcpt_conv_ln_fwd_bf16 with the conv's cached operand
    images ``pk`` (a byte buffer or None), by x.dtype.  Returns z (conv output), y and the LayerNorm statistics [2][B H W]."""
    bf = x.dtype == torch.bfloat16
    B, Cin, H, W = x.shape
    Cout, ks = w_.shape[0], w_.shape[2]
    dev = x.device
    z, y = _empty(bf)(B, Cout, H, W, dev), _empty(bf)(B, Cout, H, W, dev)
    stats = torch.empty((2, B * H * W), dtype=torch.float32, device=dev)
    # (irregular: the relu flag sits between the pointers, the bf16 form takes the (pointer, bytes) pair of the weight pack)
    _call(lib.dcpt_conv_ln_fwd_bf16 if bf else lib.dcpt_conv_ln_fwd,
          (x, w_, *(_pkargs(pk) if bf else ()), lw, lb, res, int(bool(relu)), z, y, stats[0], stats[1]), (B, H, W, Cin, Cout, ks), dev,
          _conv_ln_ws(lib, bf)(B, H, W, Cin, Cout, ks, 0))
    return z, y, stats


def _conv_ln_bwd(lib, dy, x, w_, pk, lw, z, y, stats, dx_add, has_res, relu):
    """backward of _conv_ln_fwd (dcpt_conv_ln_bwd / _bf16 by x.dtype): dx = dx_add + conv^T(dz) (dx_add may be None).  Returns dx, dw, dlnw,
    dlnb and dres (None without a residual input)."""
    bf = x.dtype == torch.bfloat16
    B, Cin, H, W = x.shape
    Cout, ks = w_.shape[0], w_.shape[2]
    dev = x.device
    dx = _empty(bf)(B, Cin, H, W, dev)
    dw = torch.empty_like(w_)
    dlw, dlb = torch.empty_like(lw), torch.empty_like(lw)
    dres = _empty(bf)(B, Cout, H, W, dev) if has_res else None
    _call(lib.dcpt_conv_ln_bwd_bf16 if bf else lib.dcpt_conv_ln_bwd,
          (dy, x, w_, *(_pkargs(pk) if bf else ()), lw, z, y, stats[0], stats[1], dx_add, dx, dw, dlw, dlb, dres),
          (B, H, W, Cin, Cout, ks, int(relu)), dev, _conv_ln_ws(lib, bf)(B, H, W, Cin, Cout, ks, 1))
    return dx, dw, dlw, dlb, dres


@_remember_gemm_mode_fp32
class _ConvLNFn(torch.autograd.Function):
    """conv(1x1 | 3x3, no bias) -> channels-first LayerNorm -> [+res] -> [ReLU]
    (Conv2d wrapper :69-103 with norm=LN; BottleneckBlock tail :227-243).  fp32 or bf16 activations (x, res, z, y and their gradients) by
    x.dtype, parameters fp32; ``packed``: the conv's PackedConvBf16 cache (bf16 activations only)."""

    @staticmethod
    def forward(ctx, x, weight, lnw, lnb, res, relu, packed):
        lib = _lib.load()
        _require_gpu(weight, lnw, lnb)   # (conv_ln / conv_ln_bf16 have checked the feature maps)
        x = _nhwc(x)
        res_ = None if res is None else _nhwc(res)
        w_, lw, lb = _contig(weight.detach()), _contig(lnw.detach()), _contig(lnb.detach())
        ctx.pk = _pk_buf(packed, weight)
        z, y, stats = _conv_ln_fwd(lib, x, w_, ctx.pk, lw, lb, res_, relu)
        ctx.save_for_backward(x, w_, lw, z, y, stats)
        ctx.relu, ctx.has_res = bool(relu), res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_, lw, z, y, stats = ctx.saved_tensors
        dy = _nhwc(_grad_cast(dy, torch.bfloat16) if x.dtype == torch.bfloat16 else dy)   # (fp32 storage: taken as it comes)
        return (*_conv_ln_bwd(lib, dy, x, w_, ctx.pk, lw, z, y, stats, None, ctx.has_res, ctx.relu), None, None)


def conv_ln(x, weight, lnw, lnb, res=None, relu=True):
    _require_gpu(x, res)
    return _ConvLNFn.apply(x, weight, lnw, lnb, res, relu, None)


def conv_ln_bf16(x, weight, lnw, lnb, res=None, relu=True, packed: PackedConvBf16 = None):
    _require_gpu_bf16(x, *([] if res is None else [res]))
    return _ConvLNFn.apply(x, weight, lnw, lnb, res, relu, packed)


@_remember_gemm_mode
class _BottleneckFn(torch.autograd.Function):
    """The whole BottleneckBlock (reference degrad_classify_arch.py:132-243 as the DCPT head instantiates it: identity shortcut) as ONE
    autograd node: relu(LN(conv1(x))) -> relu(LN(conv2(.))) -> relu(LN(conv3(.)) + x), the three conv -> LN groups through the same C
    entry points as conv_ln / conv_ln_bf16 (fp32 or bf16 activations by x.dtype).  As three nodes the block's input has two consumers
    (conv1 and the shortcut) and autograd sums their gradients with a pass of its own over the feature map -- 10 of the 18 bf16 `add`
    launches of a DCPT step; here conv3's shortcut gradient is conv1's ``dx_add`` (dcpt_conv_ln_bwd*): summed in the epilogue
    of conv1's data-gradient GEMM."""

    @staticmethod
    def forward(ctx, x, w1, lw1, lb1, w2, lw2, lb2, w3, lw3, lb3, packs=None):
        lib = _lib.load()
        bf = x.dtype == torch.bfloat16
        packs = packs if (bf and packs is not None) else (None, None, None)   # (PackedConvBf16 per conv: bf16 activations only)
        (_require_gpu_bf16 if bf else _require_gpu)(x)
        _require_gpu(w1, lw1, lb1, w2, lw2, lb2, w3, lw3, lb3)
        x = _nhwc(x)
        C_ = x.shape[1]
        ctx.fused = bf and _BottleneckFn._geometry_ok(C_, w1, lw1, lb1, w2, lw2, lb2, w3, lw3, lb3)
        if ctx.fused:
            return _BottleneckFn._forward_bf16(ctx, lib, x, ((w1, lw1, lb1), (w2, lw2, lb2), (w3, lw3, lb3)), packs)
        saved, cur, pkbufs = [x], x, []
        for (w, lw, lb, res, pck) in ((w1, lw1, lb1, None, packs[0]), (w2, lw2, lb2, None, packs[1]), (w3, lw3, lb3, x, packs[2])):
            w_, lw_, lb_ = _contig(w.detach()), _contig(lw.detach()), _contig(lb.detach())
            pkbufs.append(_pk_buf(pck, w))
            z, y, stats = _conv_ln_fwd(lib, cur, w_, pkbufs[-1], lw_, lb_, res, 1)
            saved += [w_, lw_, z, y, stats]
            cur = y
        ctx.save_for_backward(*saved)
        ctx.pkbufs = pkbufs   # (the backward of THIS forward reads the same operand images)
        return cur

    @staticmethod
    def _geometry_ok(C_, w1, lw1, lb1, w2, lw2, lb2, w3, lw3, lb3):
        """the one-call bf16 entry points assume C -> 2C (1x1) -> 2C (3x3) -> C (1x1), taken from x alone: any other width (BottleneckBlock's
        ``bottleneck_channels``) takes the per-group path"""
        C2 = 2 * C_
        return (tuple(w1.shape) == (C2, C_, 1, 1) and tuple(w2.shape) == (C2, C2, 3, 3) and tuple(w3.shape) == (C_, C2, 1, 1)
                and all(tuple(t.shape) == (C2,) for t in (lw1, lb1, lw2, lb2)) and tuple(lw3.shape) == (C_,) and tuple(lb3.shape) == (C_,))

    @staticmethod
    def _forward_bf16(ctx, lib, x, groups, packs):
        """bf16 activations: the whole block in ONE library call (dcpt_bottleneck_fwd_bf16, ABI 15: LayerNorms in the GEMM epilogues)"""
        dev = x.device
        B, C_, H, W = x.shape
        M = B * H * W
        garr = (_lib.BneckGroup * 3)()
        saved, pkbufs, keep = [x], [], []
        for k, ((w, lw, lb), pck) in enumerate(zip(groups, packs)):
            w_, lw_, lb_ = _contig(w.detach()), _contig(lw.detach()), _contig(lb.detach())
            Cout = w_.shape[0]
            z, y = _empty_nhwc_bf16(B, Cout, H, W, dev), _empty_nhwc_bf16(B, Cout, H, W, dev)
            stats = torch.empty((2, M), dtype=torch.float32, device=dev)
            pkp, pkn = _pk(pck, w)
            garr[k] = _lib.BneckGroup(w_.data_ptr(), pkp, pkn, *[t.data_ptr() for t in (lw_, lb_, z, y, stats[0], stats[1])], None, None, None)
            pkbufs.append(pck.buf if pkp is not None else None)
            saved += [w_, lw_, z, y, stats]
            keep.append(lb_)
        _call(lib.dcpt_bottleneck_fwd_bf16, (x, garr), (B, H, W, C_), dev, lib.dcpt_bottleneck_bf16_ws_bytes(B, H, W, C_, 0))
        # the LayerNorm biases last: the backward recomputes the inner ReLU masks from z with them, so an in-place update between forward and
        # backward must trip autograd's version check
        ctx.save_for_backward(*saved, *keep)
        ctx.pkbufs = pkbufs   # (the backward of THIS forward reads the same operand images)
        return saved[-2]

    @staticmethod
    def _backward_bf16(ctx, lib, dy):
        sv = ctx.saved_tensors
        x = sv[0]
        dev = x.device
        B, C_, H, W = x.shape
        g = _nhwc(_grad_cast(dy, torch.bfloat16))
        garr = (_lib.BneckGroup * 3)()
        grads = []
        for k in range(3):
            w_, lw_, z, y, stats = sv[1 + 5 * k: 6 + 5 * k]
            dw, dlw, dlb = torch.empty_like(w_), torch.empty_like(lw_), torch.empty_like(lw_)
            garr[k] = _lib.BneckGroup(w_.data_ptr(), *_pkargs(ctx.pkbufs[k]),
                                      *[t.data_ptr() for t in (lw_, sv[16 + k], z, y, stats[0], stats[1], dw, dlw, dlb)])
            grads += [dw, dlw, dlb]
        dx = _empty_nhwc_bf16(B, C_, H, W, dev)
        _call(lib.dcpt_bottleneck_bwd_bf16, (g, x, garr, dx), (B, H, W, C_), dev, lib.dcpt_bottleneck_bf16_ws_bytes(B, H, W, C_, 1))
        return (dx, *grads, None)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        if ctx.fused:
            return _BottleneckFn._backward_bf16(ctx, lib, dy)
        sv = ctx.saved_tensors
        x = sv[0]
        g = _nhwc(_grad_cast(dy, torch.bfloat16) if x.dtype == torch.bfloat16 else dy)
        grads, dshort = [None] * 9, None
        for k in (2, 1, 0):   # conv3 (its dres = the shortcut gradient), conv2, conv1 (dx = dx_add + ...)
            w_, lw_, z, y, stats = sv[1 + 5 * k: 6 + 5 * k]
            xin = x if k == 0 else sv[5 * k - 1]      # the y of group k - 1
            g, dw, dlw, dlb, dres = _conv_ln_bwd(lib, g, xin, w_, ctx.pkbufs[k], lw_, z, y, stats, dshort if k == 0 else None, k == 2, 1)
            if k == 2:
                dshort = dres
            grads[3 * k: 3 * k + 3] = [dw, dlw, dlb]
        return (g, *grads, None)


def bottleneck(x, w1, lw1, lb1, w2, lw2, lb2, w3, lw3, lb3, packs=None):
    """relu(LN(conv3(relu(LN(conv2(relu(LN(conv1(x)))))))) + x) as one autograd node (fp32 or bf16 activations); ``packs``: the three convs'
    PackedConvBf16 caches (bf16 activations)"""
    return _BottleneckFn.apply(x, w1, lw1, lb1, w2, lw2, lb2, w3, lw3, lb3, packs)


class _PatchUnfoldFn(torch.autograd.Function):
    """NCHW image -> patch rows (B, Kp, Ho, Wo) in NHWC memory, last real column = 1 (carries the conv bias);
    the unfolding half of PromptIR_DC.conv_embed (degrad_classify_arch.py:491-494)."""

    @staticmethod
    def forward(ctx, x, ksize, stride, pad):
        lib = _lib.load()
        _require_gpu(x)
        x = _contig(x)
        B, Cin, H, W = x.shape
        Kp = (Cin * ksize * ksize + 1 + 3) // 4 * 4
        Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
        A = _empty_nhwc(B, Kp, Ho, Wo, x.device)
        _call(lib.dcpt_patch_unfold, (x, A), (B, Cin, H, W, ksize, stride, pad, Kp), x.device)
        ctx.geom = (B, Cin, H, W, ksize, stride, pad, Kp)
        return A

    @staticmethod
    def backward(ctx, dA):
        lib = _lib.load()
        B, Cin, H, W, ksize, stride, pad, Kp = ctx.geom
        dA = _nhwc(dA)
        dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=dA.device)
        _call(lib.dcpt_patch_fold, (dA, dx), (B, Cin, H, W, ksize, stride, pad, Kp), dA.device)
        return dx, None, None, None


def conv_embed_ln(x, weight, bias, lnw, lnb, stride=2, pad=3):
    """Conv2d(Cin, dim, k, stride, pad) + bias -> channels-first LayerNorm (PromptIR_DC.conv_embed, :491-494):
    patch rows x [weight | bias | 0] on the MFMA GEMM, LayerNorm fused behind it."""
    dim, cin, ks, _ = weight.shape
    A = _PatchUnfoldFn.apply(x, ks, stride, pad)
    kp = A.shape[1]
    cols = [weight.reshape(dim, cin * ks * ks), bias.reshape(dim, 1)]
    if kp > cin * ks * ks + 1:
        cols.append(weight.new_zeros(dim, kp - cin * ks * ks - 1))
    wext = torch.cat(cols, dim=1).reshape(dim, kp, 1, 1)
    return conv_ln(A, wext, lnw, lnb, None, relu=False)


def _pool_relu_ws(lib, bf):
    return lib.dcpt_conv1x1_pool_relu_bf16_ws_bytes if bf else lib.dcpt_conv1x1_pool_relu_ws_bytes


@_remember_gemm_mode_fp32
class _ConvPoolReluFn(torch.autograd.Function):
    """Conv2d(1x1, bias=False) -> MaxPool2d(2,2) -> ReLU (degrad_classify_arch.py:596-602); fp32 or bf16 activations by x.dtype, the weight
    fp32; ``packed``: the conv's PackedConvBf16 cache (bf16 activations only)."""

    @staticmethod
    def forward(ctx, x, weight, packed):
        lib = _lib.load()
        _require_gpu(weight)   # (conv1x1_pool_relu / conv1x1_pool_relu_bf16 have checked the feature map)
        x = _nhwc(x)
        bf = x.dtype == torch.bfloat16
        w_ = _contig(weight.detach())
        B, Cin, H, W = x.shape
        Cout = w_.shape[0]
        dev = x.device
        z = _empty(bf)(B, Cout, H, W, dev)
        y = _empty(bf)(B, Cout, H // 2, W // 2, dev)
        ctx.pk = _pk_buf(packed, weight)
        _call(lib.dcpt_conv1x1_pool_relu_fwd_bf16 if bf else lib.dcpt_conv1x1_pool_relu_fwd, (x, w_, *(_pkargs(ctx.pk) if bf else ()), z, y),
              (B, H, W, Cin, Cout), dev, _pool_relu_ws(lib, bf)(B, H, W, Cin, Cout, 0))
        ctx.save_for_backward(x, w_, z)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_, z = ctx.saved_tensors
        bf = x.dtype == torch.bfloat16
        dy = _nhwc(_grad_cast(dy, torch.bfloat16) if bf else dy)
        B, Cin, H, W = x.shape
        Cout = w_.shape[0]
        dev = x.device
        dx = _empty(bf)(B, Cin, H, W, dev)
        dw = torch.empty_like(w_)
        _call(lib.dcpt_conv1x1_pool_relu_bwd_bf16 if bf else lib.dcpt_conv1x1_pool_relu_bwd,
              (dy, x, w_, *(_pkargs(ctx.pk) if bf else ()), z, dx, dw), (B, H, W, Cin, Cout), dev, _pool_relu_ws(lib, bf)(B, H, W, Cin, Cout, 1))
        return dx, dw, None


def conv1x1_pool_relu(x, weight):
    _require_gpu(x)
    return _ConvPoolReluFn.apply(x, weight, None)


def conv1x1_pool_relu_bf16(x, weight, packed: PackedConvBf16 = None):
    _require_gpu_bf16(x)
    return _ConvPoolReluFn.apply(x, weight, packed)


class _MixFn(torch.autograd.Function):
    """prev + softmax(mixing_weights)[idx] * feat (degrad_classify_arch.py:632-637)."""

    @staticmethod
    def forward(ctx, prev, feat, mixing_weights, idx):
        lib = _lib.load()
        _require_gpu_feat(prev, feat)
        _require_gpu(mixing_weights)
        feat = _nhwc(feat)
        prev_ = None if prev is None else _nhwc(prev)
        mw = _contig(mixing_weights.detach())
        # bf16 storage (the all-bf16 head: taps and the previous stage's output both bf16): the same arithmetic without cast passes
        bf = feat.dtype == torch.bfloat16
        if bf and prev_ is not None and prev_.dtype != torch.bfloat16:
            raise _lib.DcptHipError("mix: prev and feat must have the same storage dtype")
        out = _empty(bf)(*feat.shape, feat.device)
        _call(lib.dcpt_mix_fwd_bf16 if bf else lib.dcpt_mix_fwd, (prev_, feat, mw, mw.numel(), int(idx), out), (feat.numel(),), feat.device)
        ctx.save_for_backward(feat, mw)
        ctx.idx, ctx.has_prev = int(idx), prev is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        feat, mw = ctx.saved_tensors
        bf = feat.dtype == torch.bfloat16
        dout = _nhwc(_grad_cast(dout, feat.dtype))
        dev = feat.device
        dfeat = _empty(bf)(*feat.shape, dev)
        dmix = torch.empty_like(mw)
        _call(lib.dcpt_mix_bwd_bf16 if bf else lib.dcpt_mix_bwd, (dout, feat, mw, mw.numel(), ctx.idx, dfeat, dmix), (feat.numel(),), dev,
              lib.dcpt_mix_bwd_ws_bytes(feat.numel()))
        return (dout if ctx.has_prev else None), dfeat, dmix, None


def _tap_view(feat):
    """an fp32 (B, C, H, W) view the strided kernels can read in place (contiguous channels, strides that keep float4 alignment)
    -> (feat, sb, sh, sw); anything else is made dense NHWC first"""
    if feat.dim() != 4:
        raise ValueError(f"expected a 4-D NCHW tensor, got {tuple(feat.shape)}")
    B, Cc, H, W = feat.shape
    sb, sc, sh, sw = feat.stride()
    if (sc != 1 and Cc > 1) or sb % 4 or sh % 4 or sw % 4 or (W > 1 and sw < Cc) or feat.data_ptr() % 16:
        feat = _nhwc(feat)
        sb, sc, sh, sw = feat.stride()
    return feat, sb, sh, max(sw, Cc)


class _MixStrideFn(torch.autograd.Function):
    """prev + softmax(mixing_weights)[idx] * feat[:, :, ::s, ::s]: the mixing step of PromptIR_NoImg_DC(downsample=True)
    (degrad_classify_arch.py:634-637, F.interpolate(feature, scale_factor=1 / 2**i) in nearest mode reads source index dst * s) without
    the gather copy: dcpt_mix_stride_fwd reads the grid positions of ``feat`` through its strides (a batch slice or the strided tap of
    ``tap_split`` included).  The gradient of ``feat`` has feat's shape: the compact s * dout when stride == 1 (a pre-strided tap: its
    producer scatters), the zero-padded map written in one pass by dcpt_grid_scatter otherwise; none when feat needs none."""

    @staticmethod
    def forward(ctx, prev, feat, mixing_weights, idx, stride):
        lib = _lib.load()
        _require_gpu(prev, feat, mixing_weights)
        s = int(stride)
        feat, sb, sh, sw = _tap_view(feat)
        B, Cc, H, W = feat.shape
        if s < 1 or s & (s - 1) or H % s or W % s:
            raise ValueError(f"mix: stride {s} must be a power of two that divides the {H} x {W} map")
        prev_ = None if prev is None else _nhwc(prev)
        if prev_ is not None and tuple(prev_.shape) != (B, Cc, H // s, W // s):
            raise ValueError(f"mix: prev {tuple(prev_.shape)} does not match the tap {(B, Cc, H // s, W // s)}")
        mw = _contig(mixing_weights.detach())
        out = _empty_nhwc(B, Cc, H // s, W // s, feat.device)
        _call(lib.dcpt_mix_stride_fwd, (prev_, feat, mw, mw.numel(), int(idx), out), (B, H, W, Cc, s, sb, sh, sw), feat.device)
        ctx.save_for_backward(feat, mw)
        ctx.meta = (int(idx), prev is not None, s, sb, sh, sw)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        feat, mw = ctx.saved_tensors
        idx, has_prev, s, sb, sh, sw = ctx.meta
        B, Cc, H, W = feat.shape
        dev = feat.device
        _require_gpu(dout)
        dout = _nhwc(dout)
        dfeat = _empty_nhwc(B, Cc, H // s, W // s, dev)
        dmix = torch.empty_like(mw)
        _call(lib.dcpt_mix_stride_bwd, (dout, feat, mw, mw.numel(), idx, dfeat, dmix), (B, H, W, Cc, s, sb, sh, sw), dev,
              lib.dcpt_mix_stride_bwd_ws_bytes(dfeat.numel()))
        if not ctx.needs_input_grad[1]:
            dfeat = None
        elif s > 1:
            full = _empty_nhwc(B, Cc, H, W, dev)
            _call(lib.dcpt_grid_scatter, (dfeat, full), (B, 0, B, H, W, Cc, s), dev)
            dfeat = full
        return (dout if has_prev else None), dfeat, dmix, None, None


def mix_stride(prev, feat, mixing_weights, idx, stride=1):
    """prev + softmax(mixing_weights)[idx] * feat[:, :, ::stride, ::stride] on the strided kernels, whatever the stride (fp32)"""
    return _MixStrideFn.apply(prev, feat, mixing_weights, idx, stride)


def mix(prev, feat, mixing_weights, idx, stride=1):
    """``stride`` > 1, or an fp32 tap that is a strided view with contiguous channels (``tap_split(..., stride=s)``): read in place by
    the strided kernels; everything else is the dense node"""
    if stride == 1 and (feat.dim() != 4 or feat.dtype != torch.float32 or feat.stride(1) != 1 or _is_nhwc(feat)):
        return _MixFn.apply(prev, feat, mixing_weights, idx)
    return _MixStrideFn.apply(prev, feat, mixing_weights, idx, stride)


@_remember_gemm_mode
class _MeanPoolFCFn(torch.autograd.Function):
    """x.mean(dim=[-1,-2]) -> Linear (degrad_classify_arch.py:639-640)."""

    @staticmethod
    def forward(ctx, x, fw, fb):
        lib = _lib.load()
        _require_gpu_feat(x)
        _require_gpu(fw, fb)
        x = _nhwc(x)
        fw_, fb_ = _contig(fw.detach()), (None if fb is None else _contig(fb.detach()))
        B, Cc, H, W = x.shape
        NC = fw_.shape[0]
        dev = x.device
        pooled = torch.empty((B, Cc), dtype=torch.float32, device=dev)
        logits = torch.empty((B, NC), dtype=torch.float32, device=dev)
        bf = x.dtype == torch.bfloat16   # bf16-storage feature map: pooled in fp32 straight from it, its gradient stored in bf16
        _call(lib.dcpt_meanpool_fc_fwd_bf16 if bf else lib.dcpt_meanpool_fc_fwd, (x, fw_, fb_, pooled, logits), (B, H * W, Cc, NC), dev,
              lib.dcpt_meanpool_fc_ws_bytes(B, H * W, Cc))
        ctx.save_for_backward(pooled, fw_)
        ctx.shape, ctx.has_bias, ctx.bf = (B, Cc, H, W), fb is not None, bf
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lib = _lib.load()
        pooled, fw_ = ctx.saved_tensors
        B, Cc, H, W = ctx.shape
        NC = fw_.shape[0]
        dev = pooled.device
        dl = _contig(dlogits)
        dx = _empty(ctx.bf)(B, Cc, H, W, dev)
        dfw = torch.empty_like(fw_)
        dfb = torch.empty((NC,), dtype=torch.float32, device=dev)
        _call(lib.dcpt_meanpool_fc_bwd_bf16 if ctx.bf else lib.dcpt_meanpool_fc_bwd, (dl, pooled, fw_, dx, dfw, dfb), (B, H * W, Cc, NC), dev,
              lib.dcpt_meanpool_fc_ws_bytes(B, H * W, Cc))
        return dx, dfw, (dfb if ctx.has_bias else None)


def meanpool_fc(x, fw, fb):
    return _MeanPoolFCFn.apply(x, fw, fb)


# ------------------------------------------------------------------------------------------------
# Restormer pieces (reference basicsr/archs/restormer_arch.py)
from ._lib import GdfnParams, GdfnSaved, MdtaParams, MdtaSaved  # noqa: E402


def _conv_ws(lib, bf):
    return lib.dcpt_conv_bf16_ws_bytes if bf else lib.dcpt_conv_ws_bytes


@_remember_gemm_mode_fp32
class _ConvFn(torch.autograd.Function):
    """bias-free conv (1x1 or dense 3x3 / pad 1), NHWC -> NHWC; fp32 or bf16 features by x.dtype, the weight and its gradient fp32."""

    @staticmethod
    def forward(ctx, x, weight):
        lib = _lib.load()
        _require_gpu_feat(x)
        _require_gpu(weight)
        x = _nhwc(x)
        bf = x.dtype == torch.bfloat16
        w_ = _contig(weight.detach())
        B, Cin, H, W = x.shape
        Cout, ks = w_.shape[0], w_.shape[2]
        dev = x.device
        y = _empty(bf)(B, Cout, H, W, dev)
        _call(lib.dcpt_conv_fwd_bf16 if bf else lib.dcpt_conv_fwd, (x, w_, y), (B, H, W, Cin, Cout, ks), dev,
              _conv_ws(lib, bf)(B, H, W, Cin, Cout, ks, 0))
        ctx.save_for_backward(x, w_)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_ = ctx.saved_tensors
        bf = x.dtype == torch.bfloat16
        dy = _nhwc(_grad_strict(dy, bf))
        B, Cin, H, W = x.shape
        Cout, ks = w_.shape[0], w_.shape[2]
        dev = x.device
        dx = _empty(bf)(B, Cin, H, W, dev)
        dw = torch.empty_like(w_)
        _call(lib.dcpt_conv_bwd_bf16 if bf else lib.dcpt_conv_bwd, (dy, x, w_, dx, dw), (B, H, W, Cin, Cout, ks), dev,
              _conv_ws(lib, bf)(B, H, W, Cin, Cout, ks, 1))
        return dx, dw


def conv_nobias(x, weight):
    return _ConvFn.apply(x, weight)


def _shuffle(lib, x, up):
    x = _nhwc(x)
    bf = x.dtype == torch.bfloat16
    B, Cc, H, W = x.shape
    if up:
        y = _empty(bf)(B, Cc // 4, 2 * H, 2 * W, x.device)
        fn = lib.dcpt_pixel_shuffle_bf16 if bf else lib.dcpt_pixel_shuffle
    else:
        y = _empty(bf)(B, 4 * Cc, H // 2, W // 2, x.device)
        fn = lib.dcpt_pixel_unshuffle_bf16 if bf else lib.dcpt_pixel_unshuffle
    _call(fn, (x, y), (B, H, W, Cc), x.device)
    return y


class _PixelShuffleFn(torch.autograd.Function):
    """PixelShuffle(2) (up) / PixelUnshuffle(2) on fp32 or bf16 NHWC maps; the backward is the other one, in the forward's storage."""

    @staticmethod
    def forward(ctx, x, up):
        _require_gpu_feat(x)
        ctx.up, ctx.bf = bool(up), x.dtype == torch.bfloat16
        return _shuffle(_lib.load(), x, ctx.up)

    @staticmethod
    def backward(ctx, dy):
        (_require_gpu_bf16 if ctx.bf else _require_gpu)(dy)   # (strict in either storage; _grad_strict knows bf16 storage only)
        return _shuffle(_lib.load(), dy, not ctx.up), None


def pixel_unshuffle2(x):
    return _PixelShuffleFn.apply(x, False)


def pixel_shuffle2(x):
    return _PixelShuffleFn.apply(x, True)


class _ConcatFn(torch.autograd.Function):
    """torch.cat([a, b], 1) on NHWC maps, both fp32 or both bf16."""

    @staticmethod
    def forward(ctx, a, b):
        lib = _lib.load()
        _require_gpu_feat(a, b)
        if a.dtype != b.dtype:
            raise _lib.DcptHipError("concat_channels: a and b must have the same storage dtype")
        a, b = _nhwc(a), _nhwc(b)
        bf = a.dtype == torch.bfloat16
        B, Ca, H, W = a.shape
        Cb = b.shape[1]
        out = _empty(bf)(B, Ca + Cb, H, W, a.device)
        _call(lib.dcpt_concat_channels_bf16 if bf else lib.dcpt_concat_channels, (a, b, out), (B * H * W, Ca, Cb), a.device)
        ctx.dims, ctx.bf = (Ca, Cb), bf
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        bf = ctx.bf
        dout = _nhwc(_grad_strict(dout, bf))
        Ca, Cb = ctx.dims
        B, _, H, W = dout.shape
        da = _empty(bf)(B, Ca, H, W, dout.device)
        db = _empty(bf)(B, Cb, H, W, dout.device)
        _call(lib.dcpt_split_channels_bf16 if bf else lib.dcpt_split_channels, (dout, da, db), (B * H * W, Ca, Cb), dout.device)
        return da, db


def concat_channels(a, b):
    return _ConcatFn.apply(a, b)


# What the Restormer halves keep for backward (every saved pointer of dcpt_mdta_saved / dcpt_gdfn_saved may be NULL on its own; the
# backward entry points recompute what is missing with the forward kernels, bit-identical results):
#   "full"      everything the backward pass reads: 19 [M][C] units per block (fastest; B = 64, 128 x 128: 118-125 GB);
#   "balanced"  (DEFAULT) LN(x) of both halves, attn @ v and the GDFN gate product gelu(x1) * x2 are NOT kept -- two bandwidth passes,
#               one small batched GEMM and one depthwise-gate pass per block in backward: 13.3 units (86 GB, +6 % time);
#   "lean"      additionally the qkv conv output (one more C x 3C GEMM in backward): 10.3 units (69 GB);
#   "auto"      opt-in: ONE choice per network forward from the memory the process holds on the device when the forward starts
#               ('full' below 40 % of the device memory, 'balanced' up to 70 %, 'lean' beyond).
# The mode is explicit: ``network_g.save_mode`` in the options (ctor kwarg of Restormer / Restormer_origin) or the process default
# (set_restormer_save / DCPT_RESTORMER_SAVE); the default does NOT look at free memory -- a DDP rank or a co-resident model gets the same
# schedule, step time and peak memory as a process that has the device to itself (round-4 verdict / advisor finding).
# Measured on MI355X, Restormer B = 64, 128 x 128 (profiles/r3/extra_restormer_*.json, profiles/r5/).
import contextlib as _contextlib  # noqa: E402

_RESTORMER_MODES = ("auto", "full", "balanced", "lean")
_RESTORMER_SAVE = _os.environ.get("DCPT_RESTORMER_SAVE", "balanced")
if _RESTORMER_SAVE not in _RESTORMER_MODES:
    raise ValueError(f"DCPT_RESTORMER_SAVE={_RESTORMER_SAVE!r}: expected one of {_RESTORMER_MODES}")
_RESTORMER_SCOPED = None          # the resolved mode of the network forward that is running (restormer_save), or None
_DEV_TOTAL: Dict[int, int] = {}


def set_restormer_save(mode: str) -> str:
    """Process default: 'balanced' (initially), 'full', 'lean' or 'auto'; returns the previous default."""
    global _RESTORMER_SAVE
    if mode not in _RESTORMER_MODES:
        raise ValueError(f"restormer save mode {mode!r}: expected one of {_RESTORMER_MODES}")
    prev, _RESTORMER_SAVE = _RESTORMER_SAVE, mode
    return prev


def _resolve_restormer_mode(mode, dev) -> str:
    if mode != "auto":
        return mode
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    total = _DEV_TOTAL.get(idx)
    if total is None:
        total = _DEV_TOTAL[idx] = torch.cuda.get_device_properties(idx).total_memory
    used = torch.cuda.memory_allocated(idx) / total
    return "full" if used < 0.40 else "balanced" if used < 0.70 else "lean"


@_contextlib.contextmanager
def restormer_save(mode, dev):
    """Scope of one network forward: ``mode`` (None = the process default) is resolved ONCE here -- 'auto' looks at the device memory now,
    not block by block -- and every MDTA / GDFN half inside the scope keeps the same set of tensors."""
    global _RESTORMER_SCOPED
    mode = _RESTORMER_SAVE if mode is None else mode
    if mode not in _RESTORMER_MODES:
        raise ValueError(f"restormer save mode {mode!r}: expected one of {_RESTORMER_MODES}")
    prev, _RESTORMER_SCOPED = _RESTORMER_SCOPED, _resolve_restormer_mode(mode, dev)
    try:
        yield _RESTORMER_SCOPED
    finally:
        _RESTORMER_SCOPED = prev


def _restormer_mode(dev) -> str:
    if _RESTORMER_SCOPED is not None:
        return _RESTORMER_SCOPED
    return _resolve_restormer_mode(_RESTORMER_SAVE, dev)   # a bare MDTA / GDFN call outside a network


# Both halves run in fp32 or in bf16 activation storage, by x.dtype (restormer_bf16.hip; Restormer / Restormer_origin / PromptIR with
# act_dtype="bf16"): in bf16 storage the feature maps and the tensors the halves keep are bf16, statistics / attention matrices /
# parameters / parameter gradients fp32.  The save modes keep the same sets of tensors in both storages (bit-identical results in every
# mode).  Two things differ beyond the storage: a bf16-storage forward with no backward to come (``train`` False, decided by the caller:
# grad mode is off inside Function.forward) runs as "lean" / not full and keeps nothing, while an fp32 forward allocates what the save
# mode says whatever the grad mode; and bit 1 of the workspace queries' mode argument (everything kept: a smaller workspace) exists in
# the bf16 queries only.
def _ws_mode(bf, full, backward):
    """the mode argument of the MDTA / GDFN workspace queries: bit 0 = backward; bit 1 (bf16 queries only) = everything was kept"""
    return int(backward) | (2 if bf and full else 0)


def _mdta_saved(stats, qkv1, qkv, nrm, att, out_att, xn):
    """dcpt_mdta_saved over the forward's buffers (qkv1 / out_att / xn: None where the save mode does not keep them)"""
    return _struct(MdtaSaved, (stats[0], stats[1], qkv1, qkv, nrm, att[0], att[1], att[2], out_att, xn))


def _mdta_fns(lib, bf):
    """(forward, backward, workspace query) of the storage type"""
    return ((lib.dcpt_mdta_bf16_fwd, lib.dcpt_mdta_bf16_bwd, lib.dcpt_mdta_bf16_ws_bytes) if bf
            else (lib.dcpt_mdta_fwd, lib.dcpt_mdta_bwd, lib.dcpt_mdta_ws_bytes))


@_remember_gemm_mode_fp32
class _MDTAFn(torch.autograd.Function):
    """x + project_out(attn(LN(x)))  (restormer_arch.py:103-145, :156-157) -> dcpt_mdta_fwd / _bwd or dcpt_mdta_bf16_fwd / _bwd."""

    @staticmethod
    def forward(ctx, x, norm_w, norm_b, qkv_w, dw_w, proj_w, temperature, heads, flags, train):
        lib = _lib.load()
        _require_gpu_feat(x)
        _require_gpu(norm_w, norm_b, qkv_w, dw_w, proj_w, temperature)
        x = _nhwc(x)
        bf = x.dtype == torch.bfloat16
        ps = [None if t is None else _contig(t.detach()) for t in (norm_w, norm_b, qkv_w, dw_w, proj_w, temperature)]
        B, Cc, H, W = x.shape
        dev = x.device
        M, ch = B * H * W, Cc // heads
        nograd = bf and not train
        y = _empty(bf)(B, Cc, H, W, dev)
        stats = torch.empty((2, M), dtype=torch.float32, device=dev)
        mode = "lean" if nograd else _restormer_mode(dev)
        qkv1 = None if mode == "lean" else _empty(bf)(B, 3 * Cc, H, W, dev)
        qkv = _empty(bf)(B, 3 * Cc, H, W, dev)
        nrm = torch.empty((B, 2 * Cc), dtype=torch.float32, device=dev)
        att = torch.empty((3, B, heads, ch, ch), dtype=torch.float32, device=dev)
        out_att = None if mode != "full" else _empty(bf)(B, Cc, H, W, dev)
        xn = None if mode != "full" else _empty(bf)(B, Cc, H, W, dev)
        fwd, _, ws_bytes = _mdta_fns(lib, bf)
        _call(fwd, (_struct(MdtaParams, ps), x, y, _mdta_saved(stats, qkv1, qkv, nrm, att, out_att, xn)), (B, H, W, Cc, heads, int(flags)), dev,
              ws_bytes(B, H, W, Cc, heads, _ws_mode(bf, mode == "full", False)))
        ctx.heads, ctx.flags = heads, int(flags)
        ctx.has_bias = ps[1] is not None
        if nograd:   # nothing is kept for a backward pass that cannot happen
            return y
        kept = [t for t in (qkv1, out_att, xn) if t is not None]
        ctx.kept = (qkv1 is not None, out_att is not None, xn is not None)
        ctx.save_for_backward(x, stats, qkv, nrm, att, *kept, *[t for t in ps if t is not None])
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, stats, qkv, nrm, att, *ps = ctx.saved_tensors
        ps = list(ps)
        qkv1, out_att, xn = (ps.pop(0) if k else None for k in ctx.kept)
        if ctx.has_bias:
            norm_w, norm_b, qkv_w, dw_w, proj_w, temp = ps
        else:
            norm_w, qkv_w, dw_w, proj_w, temp = ps
            norm_b = None
        bf = x.dtype == torch.bfloat16
        dy = _nhwc(_grad_strict(dy, bf))
        B, Cc, H, W = x.shape
        dev = x.device
        dx = _empty(bf)(B, Cc, H, W, dev)
        plist = [norm_w, norm_b, qkv_w, dw_w, proj_w, temp]
        grads = [None if t is None else torch.empty_like(t) for t in plist]
        _, bwd, ws_bytes = _mdta_fns(lib, bf)
        _call(bwd, (_struct(MdtaParams, plist), _struct(MdtaParams, grads), x, _mdta_saved(stats, qkv1, qkv, nrm, att, out_att, xn), dy, dx),
              (B, H, W, Cc, ctx.heads, ctx.flags), dev, ws_bytes(B, H, W, Cc, ctx.heads, _ws_mode(bf, all(ctx.kept), True)))
        return (dx, *grads, None, None, None)


LN_BIASFREE, LN_EPS_1E5, ATTN_SOFTMAX = 1, 2, 4   # include/dcpt_hip.h: DCPT_LN_BIASFREE, DCPT_LN_EPS_1E5, DCPT_ATTN_SOFTMAX


def _wants_grad(*ts) -> bool:
    """a backward pass can follow; decided by the caller (autograd.Function.forward itself always runs with grad mode off)"""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def mdta(x, norm_w, norm_b, qkv_w, dw_w, proj_w, temperature, heads, biasfree, eps_1e5=False, softmax=False):
    """``eps_1e5`` / ``softmax``: the PromptIR variants (LayerNorm eps 1e-5, softmax instead of ReLU attention).  x and the result are
    fp32 or torch.bfloat16 NHWC maps (bf16 activation storage)."""
    flags = (LN_BIASFREE if biasfree else 0) | (LN_EPS_1E5 if eps_1e5 else 0) | (ATTN_SOFTMAX if softmax else 0)
    train = _wants_grad(x, norm_w, norm_b, qkv_w, dw_w, proj_w, temperature)
    return _MDTAFn.apply(x, norm_w, norm_b, qkv_w, dw_w, proj_w, temperature, heads, flags, train)


def _gdfn_saved(stats, u, t, xn):
    """dcpt_gdfn_saved over the forward's buffers (t / xn: None unless everything is kept)"""
    return _struct(GdfnSaved, (stats[0], stats[1], u, t, xn))


def _gdfn_fns(lib, bf):
    """(forward, backward, workspace query) of the storage type"""
    return ((lib.dcpt_gdfn_bf16_fwd, lib.dcpt_gdfn_bf16_bwd, lib.dcpt_gdfn_bf16_ws_bytes) if bf
            else (lib.dcpt_gdfn_fwd, lib.dcpt_gdfn_bwd, lib.dcpt_gdfn_ws_bytes))


@_remember_gemm_mode_fp32
class _GDFNFn(torch.autograd.Function):
    """x + project_out(gelu(x1) * x2)  (restormer_arch.py:75-100, :158) -> dcpt_gdfn_fwd / _bwd (hidden padded to a multiple of 4) or
    dcpt_gdfn_bf16_fwd / _bwd (to a multiple of 8)."""

    @staticmethod
    def forward(ctx, x, norm_w, norm_b, in_w, dw_w, out_w, flags, train):
        lib = _lib.load()
        _require_gpu_feat(x)
        _require_gpu(norm_w, norm_b, in_w, dw_w, out_w)
        x = _nhwc(x)
        bf = x.dtype == torch.bfloat16
        ps = [None if t is None else _contig(t.detach()) for t in (norm_w, norm_b, in_w, dw_w, out_w)]
        B, Cc, H, W = x.shape
        dev = x.device
        M = B * H * W
        hidden = ps[4].shape[1]
        hp = (hidden + 7) // 8 * 8 if bf else (hidden + 3) // 4 * 4
        nograd = bf and not train
        y = _empty(bf)(B, Cc, H, W, dev)
        stats = torch.empty((2, M), dtype=torch.float32, device=dev)
        full = not nograd and _restormer_mode(dev) == "full"
        u = _empty(bf)(B, 2 * hp, H, W, dev)
        t = _empty(bf)(B, hp, H, W, dev) if full else None
        xn = _empty(bf)(B, Cc, H, W, dev) if full else None
        fwd, _, ws_bytes = _gdfn_fns(lib, bf)
        _call(fwd, (_struct(GdfnParams, ps), x, y, _gdfn_saved(stats, u, t, xn)), (B, H, W, Cc, hidden, int(flags)), dev,
              ws_bytes(B, H, W, Cc, hidden, _ws_mode(bf, full, False)))
        ctx.full = full
        ctx.has_bias, ctx.flags, ctx.hidden = ps[1] is not None, int(flags), hidden
        if nograd:
            return y
        ctx.save_for_backward(x, stats, u, *([t, xn] if full else []), *[q for q in ps if q is not None])
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, stats, u, *ps = ctx.saved_tensors
        t = xn = None
        if ctx.full:
            t, xn, *ps = ps
        if ctx.has_bias:
            norm_w, norm_b, in_w, dw_w, out_w = ps
        else:
            norm_w, in_w, dw_w, out_w = ps
            norm_b = None
        bf = x.dtype == torch.bfloat16
        dy = _nhwc(_grad_strict(dy, bf))
        B, Cc, H, W = x.shape
        dev = x.device
        dx = _empty(bf)(B, Cc, H, W, dev)
        plist = [norm_w, norm_b, in_w, dw_w, out_w]
        grads = [None if q is None else torch.empty_like(q) for q in plist]
        _, bwd, ws_bytes = _gdfn_fns(lib, bf)
        _call(bwd, (_struct(GdfnParams, plist), _struct(GdfnParams, grads), x, _gdfn_saved(stats, u, t, xn), dy, dx),
              (B, H, W, Cc, ctx.hidden, ctx.flags), dev, ws_bytes(B, H, W, Cc, ctx.hidden, _ws_mode(bf, ctx.full, True)))
        return (dx, *grads, None, None)


def gdfn(x, norm_w, norm_b, in_w, dw_w, out_w, biasfree, eps_1e5=False):
    flags = (LN_BIASFREE if biasfree else 0) | (LN_EPS_1E5 if eps_1e5 else 0)
    return _GDFNFn.apply(x, norm_w, norm_b, in_w, dw_w, out_w, flags, _wants_grad(x, norm_w, norm_b, in_w, dw_w, out_w))


def mdta_bf16(x, norm_w, norm_b, qkv_w, dw_w, proj_w, temperature, heads, biasfree, eps_1e5=False, softmax=False):
    """mdta() for callers that mean bf16 activation storage: anything but a torch.bfloat16 x is an error."""
    _require_gpu_bf16(x)
    return mdta(x, norm_w, norm_b, qkv_w, dw_w, proj_w, temperature, heads, biasfree, eps_1e5, softmax)


def gdfn_bf16(x, norm_w, norm_b, in_w, dw_w, out_w, biasfree, eps_1e5=False):
    """gdfn() for callers that mean bf16 activation storage."""
    _require_gpu_bf16(x)
    return gdfn(x, norm_w, norm_b, in_w, dw_w, out_w, biasfree, eps_1e5)


# ------------------------------------------------------------------------------------------------
class _PromptMixFn(torch.autograd.Function):
    """bilinear_(H,W)( sum_l softmax(logits)[b, l] * prompt_param[l] ) as an NHWC map
    (PromptGenBlock.forward, basicsr/archs/promptir_arch.py:253-259).  ``out_bf16``: the map (and the dout that comes back) in bf16
    storage (dcpt_prompt_mix_fwd_bf16 / _bwd_bf16); logits, softmax weights, prompt_param and their gradients are fp32 in both."""

    @staticmethod
    def forward(ctx, logits, prompt_param, H, W, out_bf16):
        lib = _lib.load()
        _require_gpu(logits, prompt_param)
        lg, pp = _contig(logits.detach()), _contig(prompt_param.detach())
        B, L = lg.shape
        _, L2, D, S, S2 = pp.shape
        if L2 != L or S2 != S:
            raise ValueError(f"prompt_param {tuple(pp.shape)} does not match logits {tuple(lg.shape)}")
        dev = lg.device
        bf = bool(out_bf16)
        wsm = torch.empty((B, L), dtype=torch.float32, device=dev)
        out = _empty(bf)(B, D, H, W, dev)
        _call(lib.dcpt_prompt_mix_fwd_bf16 if bf else lib.dcpt_prompt_mix_fwd, (lg, pp, wsm, out), (B, L, D, S, H, W), dev)
        ctx.save_for_backward(pp, wsm)
        ctx.geom, ctx.bf = (B, L, D, S, H, W), bf
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        pp, wsm = ctx.saved_tensors
        B, L, D, S, H, W = ctx.geom
        dout = _nhwc(_grad_strict(dout, ctx.bf))
        dev = dout.device
        dlogits = torch.empty((B, L), dtype=torch.float32, device=dev)
        dparam = torch.empty_like(pp)
        _call(lib.dcpt_prompt_mix_bwd_bf16 if ctx.bf else lib.dcpt_prompt_mix_bwd, (dout, pp, wsm, dlogits, dparam), (B, L, D, S, H, W), dev,
              lib.dcpt_prompt_mix_bwd_ws_bytes(B, D, S))
        return dlogits, dparam, None, None, None


def prompt_mix(logits, prompt_param, H, W, out_bf16=False):
    """``out_bf16``: the map in bf16 storage (PromptIR with act_dtype="bf16"), otherwise fp32."""
    return _PromptMixFn.apply(logits, prompt_param, H, W, out_bf16)


# ------------------------------------------------------------------------------------------------
# SwinIR (include/dcpt_hip.h dcpt_swin_*, dcpt_conv3x3_res_*, dcpt_img_affine).  Token maps are (B, C, H, W) channels_last tensors: the
# reference's (B, L, C) token rows are exactly the NHWC rows.  ``grad_mode`` is decided by the caller (inside an autograd Function's
# forward grad mode is off): without it the forward keeps nothing for backward -- every intermediate lives in the workspace.
from ._lib import SwinAttnParams, SwinAttnSaved, SwinMlpParams, SwinMlpSaved  # noqa: E402


def _swin_attn_saved(stats, qkv, att, lse):
    return _struct(SwinAttnSaved, (stats[0], stats[1], qkv, att, lse))


def _swin_mlp_saved(stats, h):
    return _struct(SwinMlpSaved, (stats[0], stats[1], h))


@_remember_gemm_mode
class _SwinAttnFn(torch.autograd.Function):
    """x + proj(WMSA_shift(qkv(LN1(x))))  (swinir_arch.py SwinTransformerBlock up to its first residual, WindowAttention)."""

    @staticmethod
    def forward(ctx, x, grad_mode, heads, window, shift, norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b):
        lib = _lib.load()
        _require_gpu(x, norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b)
        x = _nhwc(x)
        ps = [_contig(t.detach()) for t in (norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b)]
        B, Cc, H, W = x.shape
        dev = x.device
        M = B * H * W
        y = _empty_nhwc(B, Cc, H, W, dev)
        sv = None
        if grad_mode:
            stats = torch.empty((2, M), dtype=torch.float32, device=dev)
            qkv = torch.empty((M, 3 * Cc), dtype=torch.float32, device=dev)
            att = torch.empty((M, Cc), dtype=torch.float32, device=dev)
            lse = torch.empty((M, heads), dtype=torch.float32, device=dev)
            sv = _swin_attn_saved(stats, qkv, att, lse)
        _call(lib.dcpt_swin_attn_fwd, (_struct(SwinAttnParams, ps), x, y, sv), (B, H, W, Cc, heads, window, shift), dev,
              lib.dcpt_swin_attn_ws_bytes(B, H, W, Cc, heads, 0))
        if grad_mode:
            ctx.save_for_backward(x, stats, qkv, att, lse, *ps)
        ctx.geom = (heads, window, shift)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, stats, qkv, att, lse, *ps = ctx.saved_tensors
        heads, window, shift = ctx.geom
        dy = _nhwc(dy)
        B, Cc, H, W = x.shape
        dev = x.device
        dx = _empty_nhwc(B, Cc, H, W, dev)
        grads = [torch.empty_like(t) for t in ps]
        _call(lib.dcpt_swin_attn_bwd, (_struct(SwinAttnParams, ps), _struct(SwinAttnParams, grads), x, _swin_attn_saved(stats, qkv, att, lse),
                                       dy, dx), (B, H, W, Cc, heads, window, shift), dev, lib.dcpt_swin_attn_ws_bytes(B, H, W, Cc, heads, 1))
        return (dx, None, None, None, None, *grads)


def swin_attn(x, norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b, heads, window, shift):
    ps = (norm_w, norm_b, qkv_w, qkv_b, proj_w, proj_b)
    return _SwinAttnFn.apply(x, _wants_grad(x, *ps), int(heads), int(window), int(shift), *ps)


@_remember_gemm_mode
class _SwinMlpFn(torch.autograd.Function):
    """x + fc2(gelu(fc1(LN2(x))))  (swinir_arch.py SwinTransformerBlock's second residual, Mlp)."""

    @staticmethod
    def forward(ctx, x, grad_mode, norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b):
        lib = _lib.load()
        _require_gpu(x, norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b)
        x = _nhwc(x)
        ps = [_contig(t.detach()) for t in (norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b)]
        B, Cc, H, W = x.shape
        dev = x.device
        M, hidden = B * H * W, ps[2].shape[0]
        y = _empty_nhwc(B, Cc, H, W, dev)
        sv = None
        if grad_mode:
            stats = torch.empty((2, M), dtype=torch.float32, device=dev)
            h = torch.empty((M, hidden), dtype=torch.float32, device=dev)
            sv = _swin_mlp_saved(stats, h)
        _call(lib.dcpt_swin_mlp_fwd, (_struct(SwinMlpParams, ps), x, y, sv), (B, H, W, Cc, hidden), dev,
              lib.dcpt_swin_mlp_ws_bytes(B, H, W, Cc, hidden, 0))
        if grad_mode:
            ctx.save_for_backward(x, stats, h, *ps)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, stats, h, *ps = ctx.saved_tensors
        dy = _nhwc(dy)
        B, Cc, H, W = x.shape
        dev = x.device
        hidden = ps[2].shape[0]
        dx = _empty_nhwc(B, Cc, H, W, dev)
        grads = [torch.empty_like(t) for t in ps]
        _call(lib.dcpt_swin_mlp_bwd, (_struct(SwinMlpParams, ps), _struct(SwinMlpParams, grads), x, _swin_mlp_saved(stats, h), dy, dx),
              (B, H, W, Cc, hidden), dev, lib.dcpt_swin_mlp_ws_bytes(B, H, W, Cc, hidden, 1))
        return (dx, None, *grads)


def swin_mlp(x, norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b):
    ps = (norm_w, norm_b, fc1_w, fc1_b, fc2_w, fc2_b)
    return _SwinMlpFn.apply(x, _wants_grad(x, *ps), *ps)


@_remember_gemm_mode
class _Conv3x3ResFn(torch.autograd.Function):
    """res + conv3x3(x) + bias, NHWC -> NHWC (the RSTB conv and conv_after_body, swinir_arch.py:634-640, :1098-1099)."""

    @staticmethod
    def forward(ctx, x, weight, bias, res):
        lib = _lib.load()
        _require_gpu(x, weight, bias, res)
        x, res = _nhwc(x), _nhwc(res)
        w_, b_ = _contig(weight.detach()), _contig(bias.detach())
        B, Cc, H, W = x.shape
        dev = x.device
        y = _empty_nhwc(B, Cc, H, W, dev)
        _call(lib.dcpt_conv3x3_res_fwd, (x, w_, b_, res, y), (B, H, W, Cc), dev, lib.dcpt_conv3x3_res_ws_bytes(B, H, W, Cc, 0))
        ctx.save_for_backward(x, w_)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_ = ctx.saved_tensors
        dy = _nhwc(dy)
        B, Cc, H, W = x.shape
        dev = x.device
        dx = _empty_nhwc(B, Cc, H, W, dev)
        dw = torch.empty_like(w_)
        db = torch.empty((Cc,), dtype=torch.float32, device=dev)
        _call(lib.dcpt_conv3x3_res_bwd, (dy, x, w_, dx, dw, db), (B, H, W, Cc), dev, lib.dcpt_conv3x3_res_ws_bytes(B, H, W, Cc, 1))
        return dx, dw, db, dy


def conv3x3_res(x, weight, bias, res):
    return _Conv3x3ResFn.apply(x, weight, bias, res)


class _ImgAffineFn(torch.autograd.Function):
    """dir 0: (x - mean) * r;  dir 1: x / r + mean   (NCHW image, swinir_arch.py:1064-1065, :1102)."""

    @staticmethod
    def forward(ctx, x, mean, r, direction):
        lib = _lib.load()
        _require_gpu(x, mean)
        x = _contig(x)
        m = _contig(mean.detach().reshape(-1))
        B, Cc, H, W = x.shape
        if m.numel() != Cc:
            raise ValueError(f"mean has {m.numel()} entries for {Cc} channels")
        y = torch.empty_like(x)
        _call(lib.dcpt_img_affine, (x, m, y), (B, Cc, H * W, float(r), int(direction)), x.device)
        ctx.geom = (float(r), int(direction))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        r, direction = ctx.geom
        dy = _contig(dy)
        B, Cc, H, W = dy.shape
        dx = torch.empty_like(dy)
        _call(lib.dcpt_img_affine, (dy, None, dx), (B, Cc, H * W, r, direction), dy.device)
        return dx, None, None, None


def img_affine(x, mean, r, direction):
    return _ImgAffineFn.apply(x, mean, r, direction)


# ------------------------------------------------------------------------------------------------
# RCAN (include/dcpt_hip.h dcpt_rcab_*, dcpt_conv3x3_ps_*).  Feature maps are (B, C, H, W) channels_last tensors.
from ._lib import RcabParams, RcabSaved  # noqa: E402


def _rcab_saved(h, t, ps_):
    """dcpt_rcab_saved: h, t and the two [B][C] rows (pooled mean, sigmoid scale) of ``ps_``"""
    return _struct(RcabSaved, (h, t, ps_[0], ps_[1]))


@_remember_gemm_mode
class _RcabFn(torch.autograd.Function):
    """x + res_scale * CA(conv2(relu(conv1(x))))  (rcan_arch.py RCAB, ChannelAttention)."""

    @staticmethod
    def forward(ctx, x, grad_mode, res_scale, conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b):
        lib = _lib.load()
        _require_gpu(x, conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b)
        x = _nhwc(x)
        ps = [_contig(t.detach()) for t in (conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b)]
        B, Cc, H, W = x.shape
        Cr = ps[4].shape[0]
        dev = x.device
        y = _empty_nhwc(B, Cc, H, W, dev)
        ws = _workspace(dev, lib.dcpt_rcab_ws_bytes(B, H, W, Cc, Cr, 0))   # (asked for before h and t, as it always was: passed inside ptrs)
        sv = None
        if grad_mode:
            h = _empty_nhwc(B, Cc, H, W, dev)
            t = _empty_nhwc(B, Cc, H, W, dev)
            ps_ = torch.empty((2, B, Cc), dtype=torch.float32, device=dev)
            sv = _rcab_saved(h, t, ps_)
        _call(lib.dcpt_rcab_fwd, (_struct(RcabParams, ps), x, y, sv, ws, ws.numel()), (B, H, W, Cc, Cr, float(res_scale)), dev)
        if grad_mode:
            ctx.save_for_backward(x, h, t, ps_, *ps)
        ctx.res_scale = float(res_scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, h, t, ps_, *ps = ctx.saved_tensors
        dy = _nhwc(dy)
        B, Cc, H, W = x.shape
        Cr = ps[4].shape[0]
        dev = x.device
        dx = _empty_nhwc(B, Cc, H, W, dev)
        grads = [torch.empty_like(p) for p in ps]
        _call(lib.dcpt_rcab_bwd, (_struct(RcabParams, ps), _struct(RcabParams, grads), x, _rcab_saved(h, t, ps_), dy, dx),
              (B, H, W, Cc, Cr, ctx.res_scale), dev, lib.dcpt_rcab_ws_bytes(B, H, W, Cc, Cr, 1))
        return (dx, None, None, *grads)


def rcab(x, conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b, res_scale=1.0):
    """one RCAB as one autograd node; ``ca1_w`` / ``ca2_w`` may keep their 1 x 1 kernel dims ([Cr][C][1][1], [C][Cr][1][1])"""
    ps = (conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b)
    return _RcabFn.apply(x, _wants_grad(x, *ps), float(res_scale), *ps)


@_remember_gemm_mode
class _Conv3x3PsFn(torch.autograd.Function):
    """PixelShuffle(r)(conv3x3(x) + bias), NHWC -> NHWC (one stage of arch_util.py Upsample)."""

    @staticmethod
    def forward(ctx, x, weight, bias, r):
        lib = _lib.load()
        _require_gpu(x, weight, bias)
        x = _nhwc(x)
        w_, b_ = _contig(weight.detach()), _contig(bias.detach())
        B, Cc, H, W = x.shape
        if tuple(w_.shape) != (r * r * Cc, Cc, 3, 3):
            raise ValueError(f"conv3x3_ps: weight {tuple(w_.shape)} for C={Cc}, r={r} (expected ({r * r * Cc}, {Cc}, 3, 3))")
        dev = x.device
        y = _empty_nhwc(B, Cc, r * H, r * W, dev)
        _call(lib.dcpt_conv3x3_ps_fwd, (x, w_, b_, y), (B, H, W, Cc, r), dev, lib.dcpt_conv3x3_ps_ws_bytes(B, H, W, Cc, r, 0))
        ctx.save_for_backward(x, w_)
        ctx.r = r
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_ = ctx.saved_tensors
        r = ctx.r
        dy = _nhwc(dy)
        B, Cc, H, W = x.shape
        dev = x.device
        dx = _empty_nhwc(B, Cc, H, W, dev)
        dw = torch.empty_like(w_)
        db = torch.empty((w_.shape[0],), dtype=torch.float32, device=dev)
        _call(lib.dcpt_conv3x3_ps_bwd, (dy, x, w_, dx, dw, db), (B, H, W, Cc, r), dev, lib.dcpt_conv3x3_ps_ws_bytes(B, H, W, Cc, r, 1))
        return dx, dw, db, None


def conv3x3_ps(x, weight, bias, r):
    return _Conv3x3PsFn.apply(x, weight, bias, int(r))


# RCAN on bf16 activation storage (include/dcpt_hip.h dcpt_rcab_fwd_bf16, dcpt_conv3x3_res_fwd_bf16, dcpt_conv3x3_ps_fwd_bf16): forward only.
# Feature maps are torch.bfloat16 channels_last, parameters fp32; ``packed*``: the conv's PackedConvBf16 cache (without it the call packs).
def _inference_only(name, *ts, what="bf16 storage for RCAN"):
    if _wants_grad(*ts):
        raise NotImplementedError(f"{name}: {what} is inference-only (there is no backward pass); run it under torch.no_grad()")


def rcab_bf16(x, conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b, res_scale=1.0, packed1: PackedConvBf16 = None,
              packed2: PackedConvBf16 = None):
    """bf16(x + res_scale * CA(conv2(relu(conv1(x)))))  (rcan_arch.py RCAB, ChannelAttention); h, t and y are rounded to bf16 where they are
    stored, the pooled mean (of the fp32 t), the CA FCs and the sigmoid are fp32"""
    lib = _lib.load()
    ps = (conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b)
    _require_gpu_bf16(x)
    _require_gpu(*ps)
    _inference_only("rcab_bf16", x, *ps)
    x = _nhwc(x)
    ps_ = [_contig(t.detach()) for t in ps]
    B, Cc, H, W = x.shape
    Cr = ps_[4].shape[0]
    if tuple(ps_[0].shape) != (Cc, Cc, 3, 3) or tuple(ps_[2].shape) != (Cc, Cc, 3, 3) or ps_[4].numel() != Cr * Cc or ps_[6].numel() != Cr * Cc:
        raise ValueError(f"rcab_bf16: parameter shapes do not fit C={Cc} (conv {tuple(ps_[0].shape)} / {tuple(ps_[2].shape)}, CA {tuple(ps_[4].shape)})")
    dev = x.device
    y = _empty_nhwc_bf16(B, Cc, H, W, dev)
    nws = _check_ws("rcab_bf16", lib.dcpt_rcab_bf16_ws_bytes(B, H, W, Cc, Cr), f"B={B} H={H} W={W} C={Cc} Cr={Cr}; C % 8 == 0")
    _call(lib.dcpt_rcab_fwd_bf16, (_struct(RcabParams, ps_), *_pk(packed1, conv1_w), *_pk(packed2, conv2_w), x, y),
          (B, H, W, Cc, Cr, float(res_scale)), dev, nws)
    return y


def conv3x3_res_bf16(x, weight, bias, res, packed: PackedConvBf16 = None):
    """bf16(res + conv3x3(x) + bias): RCAN's group conv and conv_after_body on bf16 maps"""
    lib = _lib.load()
    _require_gpu_bf16(x, res)
    _require_gpu(weight, bias)
    _inference_only("conv3x3_res_bf16", x, res, weight, bias)
    x, res = _nhwc(x), _nhwc(res)
    w_, b_ = _contig(weight.detach()), _contig(bias.detach())
    B, Cc, H, W = x.shape
    _check_conv_weight("conv3x3_res_bf16", w_, b_, Cc, Cc)
    if res.shape != x.shape:
        raise ValueError(f"conv3x3_res_bf16: residual {tuple(res.shape)} for a map {tuple(x.shape)}")
    dev = x.device
    y = _empty_nhwc_bf16(B, Cc, H, W, dev)
    nws = _check_ws("conv3x3_res_bf16", lib.dcpt_conv3x3_res_bf16_ws_bytes(B, H, W, Cc), f"B={B} H={H} W={W} C={Cc}; C % 8 == 0")
    _call(lib.dcpt_conv3x3_res_fwd_bf16, (x, w_, *_pk(packed, weight), b_, res, y), (B, H, W, Cc), dev, nws)
    return y


def conv3x3_ps_bf16(x, weight, bias, r, packed: PackedConvBf16 = None):
    """bf16(PixelShuffle(r)(conv3x3(x) + bias)), r in {2, 3}: one stage of arch_util.py Upsample on bf16 maps"""
    lib = _lib.load()
    r = int(r)
    _require_gpu_bf16(x)
    _require_gpu(weight, bias)
    _inference_only("conv3x3_ps_bf16", x, weight, bias)
    x = _nhwc(x)
    w_, b_ = _contig(weight.detach()), _contig(bias.detach())
    B, Cc, H, W = x.shape
    _check_conv_weight("conv3x3_ps_bf16", w_, b_, r * r * Cc, Cc)
    dev = x.device
    # (the workspace is asked for before y, as it always was: passed inside ptrs)
    ws = _workspace(dev, _check_ws("conv3x3_ps_bf16", lib.dcpt_conv3x3_ps_bf16_ws_bytes(B, H, W, Cc, r), f"B={B} H={H} W={W} C={Cc} r={r}; C % 8 == 0, r 2 or 3"))
    y = _empty_nhwc_bf16(B, Cc, r * H, r * W, dev)
    _call(lib.dcpt_conv3x3_ps_fwd_bf16, (x, w_, *_pk(packed, weight), b_, y, ws, ws.numel()), (B, H, W, Cc, r), dev)
    return y


# ------------------------------------------------------------------------------------------------
# SwinIR on bf16 activation storage (include/dcpt_hip.h dcpt_swin_attn_fwd_bf16, dcpt_swin_mlp_fwd_bf16, dcpt_ln_pad_fwd_bf16): forward only, on
# PADDED rows -- maps are torch.bfloat16 channels_last (B, Cp, H, W) with Cp = C rounded up to a multiple of 8 and exact zeros in the pad
# channels; the operands (zero-padded fp32 vectors, bf16 weight images) are built by the caller (basicsr/archs/swinir_arch.py) once per
# parameter version and kept in a SwinPackBf16.
from ._lib import SwinAttnBf16Params, SwinMlpBf16Params  # noqa: E402


class SwinPackBf16:
    """Cache of ONE module's padded operands for the bf16 SwinIR path: ``t`` maps names to tensors, rebuilt by ``refresh`` when a parameter's
    address or ``_version`` (or the pack generation) has changed -- the staleness rule of PackedConvBf16.  ``conv``: the PackedConvBf16 of the
    module's padded 3 x 3 weight ``t['w']`` where it has one.  A plain attribute of its module: not part of the state_dict."""

    def __init__(self):
        self.key = None
        self.t = {}
        self.conv = None
        self.stream = None
        self.event = None

    def __deepcopy__(self, memo):   # a copied module starts with an empty cache of its own
        return type(self)()

    def __reduce__(self):
        return (type(self), ())

    @staticmethod
    def key_of(params):
        return (_PACK_GENERATION,) + tuple((p.data_ptr(), p._version, p.device) for p in params)

    def refresh(self, params, build) -> bool:
        """rebuild ``t`` = build() if stale; True if it was.  ``build`` runs torch ops on the parameters' device: load-time work."""
        key = self.key_of(params)
        if key == self.key:
            if self.stream is not None and self.stream != _stream(params[0].device):
                torch.cuda.current_stream(params[0].device).wait_event(self.event)
            return False
        with torch.no_grad():
            self.t = build()
        if self.conv is not None:
            self.conv.key = None   # (a new padded weight may reuse the old one's address)
        self.key = key
        if params[0].is_cuda:
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(params[0].device))
            self.stream = _stream(params[0].device)
        return True


def _swin_inference_only(name, *ts):
    if _wants_grad(*ts):
        raise NotImplementedError(f"{name}: bf16 storage for SwinIR is inference-only (there is no backward pass); run it under torch.no_grad()")


def _padded_map(name, x, C_):
    x = _nhwc(x)
    Cp = x.shape[1]
    if not 0 < C_ <= Cp or Cp % 8:
        raise ValueError(f"{name}: a map of {Cp} channels for C={C_} (C <= Cp, Cp % 8 == 0)")
    return x, Cp


def ln_pad_bf16(x, weight_p, bias_p, C_, eps=1e-5):
    """bf16(LayerNorm over the first C_ channels of every pixel * w + b), pad channels written as 0; weight_p / bias_p fp32 [Cp]"""
    lib = _lib.load()
    _require_gpu_bf16(x)
    _require_gpu(weight_p, bias_p)
    _swin_inference_only("ln_pad_bf16", x, weight_p, bias_p)
    x, Cp = _padded_map("ln_pad_bf16", x, int(C_))
    if tuple(weight_p.shape) != (Cp,) or tuple(bias_p.shape) != (Cp,):
        raise ValueError(f"ln_pad_bf16: weight {tuple(weight_p.shape)} / bias {tuple(bias_p.shape)} for Cp={Cp}")
    B, _, H, W = x.shape
    y = _empty_nhwc_bf16(B, Cp, H, W, x.device)
    _call(lib.dcpt_ln_pad_fwd_bf16, (x, _contig(weight_p), _contig(bias_p), y), (B * H * W, int(C_), Cp, float(eps)), x.device)
    return y


def _swin_operands(name, ops, shapes):
    ops = [_contig(t.detach()) for t in ops]
    for t, (shape, dtype) in zip(ops, shapes):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_cuda:
            raise ValueError(f"{name}: operand {tuple(t.shape)} {t.dtype} on {t.device} (expected {shape} {dtype} on the device)")
    return ops


def swin_attn_bf16(x, ops, C_, heads, hdp, window, shift):
    """bf16(x + proj(WMSA(qkv(LN1(x))))) on padded rows; ``ops`` = (norm_w [Cp], norm_b [Cp], qkv_w bf16 [3 heads hdp][Cp], qkv_b [3 heads hdp],
    proj_w bf16 [Cp][heads hdp], proj_b [Cp]), zero-padded (dcpt_swin_attn_bf16_params)"""
    lib = _lib.load()
    _require_gpu_bf16(x)
    _swin_inference_only("swin_attn_bf16", x, *ops)
    C_, heads, hdp, window, shift = int(C_), int(heads), int(hdp), int(window), int(shift)
    x, Cp = _padded_map("swin_attn_bf16", x, C_)
    HD, f32, bf = heads * hdp, torch.float32, torch.bfloat16
    ops = _swin_operands("swin_attn_bf16", ops, [((Cp,), f32), ((Cp,), f32), ((3 * HD, Cp), bf), ((3 * HD,), f32), ((Cp, HD), bf), ((Cp,), f32)])
    B, _, H, W = x.shape
    dev = x.device
    y = _empty_nhwc_bf16(B, Cp, H, W, dev)
    nws = _check_ws("swin_attn_bf16", lib.dcpt_swin_attn_bf16_ws_bytes(B, H, W, C_, Cp, heads, hdp, window),
                    f"B={B} H={H} W={W} C={C_} Cp={Cp} heads={heads} hdp={hdp} window={window}")
    _call(lib.dcpt_swin_attn_fwd_bf16, (_struct(SwinAttnBf16Params, ops), x, y), (B, H, W, C_, Cp, heads, hdp, window, shift), dev, nws)
    return y


def swin_mlp_bf16(x, ops, C_):
    """bf16(x + fc2(gelu(fc1(LN2(x))))) on padded rows; ``ops`` = (norm_w [Cp], norm_b [Cp], fc1_w bf16 [hidden][Cp], fc1_b [hidden],
    fc2_w bf16 [Cp][hidden], fc2_b [Cp]) (dcpt_swin_mlp_bf16_params)"""
    lib = _lib.load()
    _require_gpu_bf16(x)
    _swin_inference_only("swin_mlp_bf16", x, *ops)
    C_ = int(C_)
    x, Cp = _padded_map("swin_mlp_bf16", x, C_)
    hidden, f32, bf = int(ops[3].numel()), torch.float32, torch.bfloat16
    ops = _swin_operands("swin_mlp_bf16", ops, [((Cp,), f32), ((Cp,), f32), ((hidden, Cp), bf), ((hidden,), f32), ((Cp, hidden), bf), ((Cp,), f32)])
    B, _, H, W = x.shape
    dev = x.device
    y = _empty_nhwc_bf16(B, Cp, H, W, dev)
    nws = _check_ws("swin_mlp_bf16", lib.dcpt_swin_mlp_bf16_ws_bytes(B, H, W, C_, Cp, hidden), f"B={B} H={H} W={W} C={C_} Cp={Cp} hidden={hidden}")
    _call(lib.dcpt_swin_mlp_fwd_bf16, (_struct(SwinMlpBf16Params, ops), x, y), (B, H, W, C_, Cp, hidden), dev, nws)
    return y


# ------------------------------------------------------------------------------------------------
# RCAN / SwinIR on bf16 maps around an fp32 residual stream (include/dcpt_hip.h, the *_bf16_res32 entry points): forward only.  The stream is
# a torch.float32 channels_last map (SwinIR: padded to Cp), its image a torch.bfloat16 map of the same shape; operands as for the bf16 ops.
class Stream32(NamedTuple):
    """what the blocks of a bf16_res32 network hand on: the fp32 residual stream and its bf16 image (None where no conv will read it)"""
    s: torch.Tensor
    sb: Optional[torch.Tensor]


def _require_stream(name, s, sb=None):
    _require_gpu(s)
    s = _nhwc(s)
    if sb is None:
        return s, None
    _require_gpu_bf16(sb)
    sb = _nhwc(sb)
    if sb.shape != s.shape:
        raise ValueError(f"{name}: bf16 image {tuple(sb.shape)} of a stream {tuple(s.shape)}")
    return s, sb


def rcab_bf16_res32(s, sb, conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b, res_scale=1.0, packed1: PackedConvBf16 = None,
                    packed2: PackedConvBf16 = None):
    """(S', bf16(S')) with S' = S + res_scale * CA(conv2(relu(conv1(Sb)))) in fp32: rcab_bf16 with the residual map ``s`` kept in fp32 and the
    convs reading its bf16 image ``sb``"""
    lib = _lib.load()
    ps = (conv1_w, conv1_b, conv2_w, conv2_b, ca1_w, ca1_b, ca2_w, ca2_b)
    _require_gpu(*ps)
    _inference_only("rcab_bf16_res32", s, sb, *ps)
    s, sb = _require_stream("rcab_bf16_res32", s, sb)
    ps_ = [_contig(t.detach()) for t in ps]
    B, Cc, H, W = s.shape
    Cr = ps_[4].shape[0]
    if tuple(ps_[0].shape) != (Cc, Cc, 3, 3) or tuple(ps_[2].shape) != (Cc, Cc, 3, 3) or ps_[4].numel() != Cr * Cc or ps_[6].numel() != Cr * Cc:
        raise ValueError(f"rcab_bf16_res32: parameter shapes do not fit C={Cc} (conv {tuple(ps_[0].shape)} / {tuple(ps_[2].shape)}, CA {tuple(ps_[4].shape)})")
    dev = s.device
    y, yb = _empty_nhwc(B, Cc, H, W, dev), _empty_nhwc_bf16(B, Cc, H, W, dev)
    nws = _check_ws("rcab_bf16_res32", lib.dcpt_rcab_bf16_res32_ws_bytes(B, H, W, Cc, Cr), f"B={B} H={H} W={W} C={Cc} Cr={Cr}; C % 8 == 0")
    _call(lib.dcpt_rcab_fwd_bf16_res32, (_struct(RcabParams, ps_), *_pk(packed1, conv1_w), *_pk(packed2, conv2_w), s, sb, y, yb),
          (B, H, W, Cc, Cr, float(res_scale)), dev, nws)
    return y, yb


def conv3x3_res_bf16_res32(x, weight, bias, res, packed: PackedConvBf16 = None, out_f32=True, out_bf16=False):
    """v = res + conv3x3(x) + bias with x bf16 and the residual ``res`` fp32, from the fp32 accumulator; returns (v or None, bf16(v) or None)
    as ``out_f32`` / ``out_bf16`` ask (at least one)"""
    lib = _lib.load()
    _require_gpu_bf16(x)
    _require_gpu(weight, bias)
    _inference_only("conv3x3_res_bf16_res32", x, res, weight, bias)
    if not (out_f32 or out_bf16):
        raise ValueError("conv3x3_res_bf16_res32: no output asked for")
    res, x = _require_stream("conv3x3_res_bf16_res32", res, x)
    w_, b_ = _contig(weight.detach()), _contig(bias.detach())
    B, Cc, H, W = x.shape
    _check_conv_weight("conv3x3_res_bf16_res32", w_, b_, Cc, Cc)
    dev = x.device
    y = _empty_nhwc(B, Cc, H, W, dev) if out_f32 else None
    yb = _empty_nhwc_bf16(B, Cc, H, W, dev) if out_bf16 else None
    nws = _check_ws("conv3x3_res_bf16_res32", lib.dcpt_conv3x3_res_bf16_res32_ws_bytes(B, H, W, Cc), f"B={B} H={H} W={W} C={Cc}; C % 8 == 0")
    _call(lib.dcpt_conv3x3_res_fwd_bf16_res32, (x, w_, *_pk(packed, weight), b_, res, y, yb), (B, H, W, Cc), dev, nws)
    return y, yb


def ln_pad_bf16_res32(x, weight_p, bias_p, C_, eps=1e-5):
    """ln_pad_bf16 of an fp32 padded map (the residual stream): the statistics see the unrounded values, the output is bf16"""
    lib = _lib.load()
    _require_gpu(x, weight_p, bias_p)
    _swin_inference_only("ln_pad_bf16_res32", x, weight_p, bias_p)
    x, Cp = _padded_map("ln_pad_bf16_res32", x, int(C_))
    if tuple(weight_p.shape) != (Cp,) or tuple(bias_p.shape) != (Cp,):
        raise ValueError(f"ln_pad_bf16_res32: weight {tuple(weight_p.shape)} / bias {tuple(bias_p.shape)} for Cp={Cp}")
    B, _, H, W = x.shape
    y = _empty_nhwc_bf16(B, Cp, H, W, x.device)
    _call(lib.dcpt_ln_pad_fwd_bf16_res32, (x, _contig(weight_p), _contig(bias_p), y), (B * H * W, int(C_), Cp, float(eps)), x.device)
    return y


def _inplace_layout(name, x, inplace):
    """an in-place update needs the caller's own dense NHWC memory: any other layout would be copied first and the copy updated"""
    if inplace and (x.dim() != 4 or _nhwc(x) is not x):
        raise ValueError(f"{name}: inplace=True needs a dense channels_last map (got shape {tuple(x.shape)}, strides {x.stride()})")


def swin_attn_bf16_res32(x, ops, C_, heads, hdp, window, shift, inplace=False):
    """x + proj(WMSA(qkv(LN1(x)))) in fp32 on padded rows: swin_attn_bf16 with the residual map fp32 in and out (``ops`` as there).
    ``inplace``: the result overwrites x (the entry point allows y == x; x must be dense channels_last, else ValueError) -- for a caller that
    owns x and keeps no other use of it"""
    lib = _lib.load()
    _require_gpu(x)
    _swin_inference_only("swin_attn_bf16_res32", x, *ops)
    C_, heads, hdp, window, shift = int(C_), int(heads), int(hdp), int(window), int(shift)
    _inplace_layout("swin_attn_bf16_res32", x, inplace)
    x, Cp = _padded_map("swin_attn_bf16_res32", x, C_)
    HD, f32, bf = heads * hdp, torch.float32, torch.bfloat16
    ops = _swin_operands("swin_attn_bf16_res32", ops, [((Cp,), f32), ((Cp,), f32), ((3 * HD, Cp), bf), ((3 * HD,), f32), ((Cp, HD), bf), ((Cp,), f32)])
    B, _, H, W = x.shape
    dev = x.device
    y = x if inplace else _empty_nhwc(B, Cp, H, W, dev)
    nws = _check_ws("swin_attn_bf16_res32", lib.dcpt_swin_attn_bf16_res32_ws_bytes(B, H, W, C_, Cp, heads, hdp, window),
                    f"B={B} H={H} W={W} C={C_} Cp={Cp} heads={heads} hdp={hdp} window={window}")
    _call(lib.dcpt_swin_attn_fwd_bf16_res32, (_struct(SwinAttnBf16Params, ops), x, y), (B, H, W, C_, Cp, heads, hdp, window, shift), dev, nws)
    return y


def swin_mlp_bf16_res32(x, ops, C_, out_bf16=False, inplace=False):
    """(y, bf16(y) or None) with y = x + fc2(gelu(fc1(LN2(x)))) in fp32 on padded rows (``ops`` as swin_mlp_bf16's); ``out_bf16``: also the
    bf16 image, the operand of the conv that follows an RSTB's last block; ``inplace``: y overwrites x, as swin_attn_bf16_res32's"""
    lib = _lib.load()
    _require_gpu(x)
    _swin_inference_only("swin_mlp_bf16_res32", x, *ops)
    C_ = int(C_)
    _inplace_layout("swin_mlp_bf16_res32", x, inplace)
    x, Cp = _padded_map("swin_mlp_bf16_res32", x, C_)
    hidden, f32, bf = int(ops[3].numel()), torch.float32, torch.bfloat16
    ops = _swin_operands("swin_mlp_bf16_res32", ops, [((Cp,), f32), ((Cp,), f32), ((hidden, Cp), bf), ((hidden,), f32), ((Cp, hidden), bf), ((Cp,), f32)])
    B, _, H, W = x.shape
    dev = x.device
    y = x if inplace else _empty_nhwc(B, Cp, H, W, dev)
    yb = _empty_nhwc_bf16(B, Cp, H, W, dev) if out_bf16 else None
    nws = _check_ws("swin_mlp_bf16_res32", lib.dcpt_swin_mlp_bf16_res32_ws_bytes(B, H, W, C_, Cp, hidden), f"B={B} H={H} W={W} C={C_} Cp={Cp} hidden={hidden}")
    _call(lib.dcpt_swin_mlp_fwd_bf16_res32, (_struct(SwinMlpBf16Params, ops), x, y, yb), (B, H, W, C_, Cp, hidden), dev, nws)
    return y, yb


# ------------------------------------------------------------------------------------------------
# SwinIR super-resolution tail and the "3conv" residual (include/dcpt_hip.h dcpt_conv3x3_act_*, dcpt_up2_conv3x3_act_*,
# dcpt_conv3x3_ps_out_*, dcpt_conv3conv_res_*).
from ._lib import Conv3convParams  # noqa: E402


def _check_conv_weight(name, w_, b_, cout, cin, k=3):
    if tuple(w_.shape) != (cout, cin, k, k) or tuple(b_.shape) != (cout,):
        raise ValueError(f"{name}: weight {tuple(w_.shape)} / bias {tuple(b_.shape)} (expected ({cout}, {cin}, {k}, {k}) / ({cout},))")


def _check_ws(name, nbytes, what):
    if nbytes == 0:
        raise ValueError(f"{name}: unsupported arguments ({what})")
    return nbytes


@_remember_gemm_mode
class _Conv3x3ActFn(torch.autograd.Function):
    """lrelu(conv3x3(x) + bias, slope), NHWC -> NHWC, Cin != Cout allowed; ``up2``: the conv runs over the nearest-2x up-sampling of x,
    which is never materialised (swinir_arch.py:983-985, :1085-1100)."""

    @staticmethod
    def forward(ctx, x, weight, bias, slope, up2):
        lib = _lib.load()
        _require_gpu(x, weight, bias)
        x = _nhwc(x)
        w_, b_ = _contig(weight.detach()), _contig(bias.detach())
        B, Cin, H, W = x.shape
        Cout = w_.shape[0]
        name = "up2_conv3x3_act" if up2 else "conv3x3_act"
        _check_conv_weight(name, w_, b_, Cout, Cin)
        if up2 and Cout != Cin:
            raise ValueError(f"up2_conv3x3_act: C -> C only (weight {tuple(w_.shape)})")
        if not 0.0 <= slope <= 1.0:
            raise ValueError(f"{name}: slope {slope} outside [0, 1]")
        dev = x.device
        what = f"B={B} H={H} W={W} Cin={Cin} Cout={Cout}: channels must be multiples of 4"
        if up2:
            y = _empty_nhwc(B, Cout, 2 * H, 2 * W, dev)
            _call(lib.dcpt_up2_conv3x3_act_fwd, (x, w_, b_, y), (B, H, W, Cin, slope), dev,
                  _check_ws(name, lib.dcpt_up2_conv3x3_act_ws_bytes(B, H, W, Cin, 0), what))
        else:
            y = _empty_nhwc(B, Cout, H, W, dev)
            _call(lib.dcpt_conv3x3_act_fwd, (x, w_, b_, y), (B, H, W, Cin, Cout, slope), dev,
                  _check_ws(name, lib.dcpt_conv3x3_act_ws_bytes(B, H, W, Cin, Cout, 0), what))
        ctx.save_for_backward(x, y, w_)
        ctx.geom = (slope, up2)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y, w_ = ctx.saved_tensors
        slope, up2 = ctx.geom
        dy = _nhwc(dy)
        B, Cin, H, W = x.shape
        Cout = w_.shape[0]
        dev = x.device
        dx = _empty_nhwc(B, Cin, H, W, dev)
        dw = torch.empty_like(w_)
        db = torch.empty((Cout,), dtype=torch.float32, device=dev)
        if up2:
            _call(lib.dcpt_up2_conv3x3_act_bwd, (dy, x, y, w_, dx, dw, db), (B, H, W, Cin, slope), dev,
                  lib.dcpt_up2_conv3x3_act_ws_bytes(B, H, W, Cin, 1))
        else:
            _call(lib.dcpt_conv3x3_act_bwd, (dy, x, y, w_, dx, dw, db), (B, H, W, Cin, Cout, slope), dev,
                  lib.dcpt_conv3x3_act_ws_bytes(B, H, W, Cin, Cout, 1))
        return dx, dw, db, None, None


def conv3x3_act(x, weight, bias, slope=0.01):
    """lrelu(conv3x3(x) + bias, slope); ``slope=1`` is the plain biased conv"""
    return _Conv3x3ActFn.apply(x, weight, bias, float(slope), False)


def up2_conv3x3_act(x, weight, bias, slope=0.2):
    """lrelu(conv3x3(nearest2x(x)) + bias, slope), (B, C, H, W) -> (B, C, 2H, 2W)"""
    return _Conv3x3ActFn.apply(x, weight, bias, float(slope), True)


@_remember_gemm_mode
class _Conv3x3PsOutFn(torch.autograd.Function):
    """PixelShuffle(r)(conv3x3(x) + bias), features NHWC -> image NCHW (UpsampleOneStep, swinir_arch.py:771-787)."""

    @staticmethod
    def forward(ctx, x, weight, bias, r):
        lib = _lib.load()
        _require_gpu(x, weight, bias)
        x = _nhwc(x)
        w_, b_ = _contig(weight.detach()), _contig(bias.detach())
        B, Cc, H, W = x.shape
        N = w_.shape[0]
        if r < 1 or N % (r * r):
            raise ValueError(f"conv3x3_ps_out: {N} conv channels are not a multiple of r^2 = {r * r}")
        _check_conv_weight("conv3x3_ps_out", w_, b_, N, Cc)
        Cimg = N // (r * r)
        dev = x.device
        nws = _check_ws("conv3x3_ps_out", lib.dcpt_conv3x3_ps_out_ws_bytes(B, H, W, Cc, Cimg, r, 0),
                        f"C={Cc} Cimg={Cimg} r={r}: C a multiple of 4, at most 4 image channels, r in 2, 3, 4")
        y = torch.empty((B, Cimg, r * H, r * W), dtype=torch.float32, device=dev)
        _call(lib.dcpt_conv3x3_ps_out_fwd, (x, w_, b_, y), (B, H, W, Cc, Cimg, r), dev, nws)
        ctx.save_for_backward(x, w_)
        ctx.geom = (Cimg, r)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w_ = ctx.saved_tensors
        Cimg, r = ctx.geom
        dy = _contig(dy)
        B, Cc, H, W = x.shape
        dev = x.device
        dx = _empty_nhwc(B, Cc, H, W, dev)
        dw = torch.empty_like(w_)
        db = torch.empty((w_.shape[0],), dtype=torch.float32, device=dev)
        _call(lib.dcpt_conv3x3_ps_out_bwd, (dy, x, w_, dx, dw, db), (B, H, W, Cc, Cimg, r), dev,
              lib.dcpt_conv3x3_ps_out_ws_bytes(B, H, W, Cc, Cimg, r, 1))
        return dx, dw, db, None


def conv3x3_ps_out(x, weight, bias, r):
    return _Conv3x3PsOutFn.apply(x, weight, bias, int(r))


@_remember_gemm_mode
class _Conv3convResFn(torch.autograd.Function):
    """res + conv3x3(lrelu(conv1x1(lrelu(conv3x3(x))))), slopes 0.2, C -> C/4 -> C/4 -> C (resi_connection="3conv",
    swinir_arch.py:608-616, :969-977)."""

    @staticmethod
    def forward(ctx, x, grad_mode, res, w1, b1, w2, b2, w3, b3):
        lib = _lib.load()
        _require_gpu(x, res, w1, b1, w2, b2, w3, b3)
        x, res = _nhwc(x), _nhwc(res)
        ps = [_contig(t.detach()) for t in (w1, b1, w2, b2, w3, b3)]
        B, Cc, H, W = x.shape
        Cq = Cc // 4
        if res.shape != x.shape:
            raise ValueError(f"conv3conv_res: residual {tuple(res.shape)} for input {tuple(x.shape)}")
        _check_conv_weight("conv3conv_res conv.0", ps[0], ps[1], Cq, Cc)
        _check_conv_weight("conv3conv_res conv.2", ps[2], ps[3], Cq, Cq, 1)
        _check_conv_weight("conv3conv_res conv.4", ps[4], ps[5], Cc, Cq)
        dev = x.device
        nws = _check_ws("conv3conv_res", lib.dcpt_conv3conv_res_ws_bytes(B, H, W, Cc, 0), f"C={Cc} must be a multiple of 16")
        y = _empty_nhwc(B, Cc, H, W, dev)
        a1 = a2 = None
        if grad_mode:
            a1, a2 = _empty_nhwc(B, Cq, H, W, dev), _empty_nhwc(B, Cq, H, W, dev)
        _call(lib.dcpt_conv3conv_res_fwd, (_struct(Conv3convParams, ps), x, res, y, a1, a2), (B, H, W, Cc), dev, nws)
        if grad_mode:
            ctx.save_for_backward(x, a1, a2, *ps)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, a1, a2, *ps = ctx.saved_tensors
        dy = _nhwc(dy)
        B, Cc, H, W = x.shape
        dev = x.device
        dx = _empty_nhwc(B, Cc, H, W, dev)
        grads = [torch.empty_like(p) for p in ps]
        _call(lib.dcpt_conv3conv_res_bwd, (_struct(Conv3convParams, ps), _struct(Conv3convParams, grads), x, a1, a2, dy, dx), (B, H, W, Cc), dev,
              lib.dcpt_conv3conv_res_ws_bytes(B, H, W, Cc, 1))
        return (dx, None, dy, *grads)


def conv3conv_res(x, w1, b1, w2, b2, w3, b3, res):
    """the "3conv" residual as one autograd node; ``w2`` keeps its 1 x 1 kernel dims ([Cq][Cq][1][1])"""
    ps = (w1, b1, w2, b2, w3, b3)
    return _Conv3convResFn.apply(x, _wants_grad(x, res, *ps), res, *ps)


# ------------------------------------------------------------------------------------------------
# Validation metrics (include/dcpt_hip.h dcpt_imgmetric): the sums behind PSNR / SSIM of NCHW image pairs, no autograd, no host sync.
METRIC_TILE = (16, 32)   # (TH, TW) of dcpt_amd/csrc/kernels.h: SSIM-map positions per workgroup (the tests aim at the tile edges)
_METRIC_Y, _METRIC_SSIM, _METRIC_RANGE1 = 1, 2, 4


def image_metric_sums(img, img2, crop_border=0, test_y_channel=False, image_range=255, ssim=True):
    """``img`` / ``img2``: (B, C, H, W) fp32 device tensors in [0, 1], C in {1, 3}.  Returns ``(sse, ssim_sums)`` as device tensors, nothing
    is synchronised: ``sse`` (B,) is the squared error per image after quantisation / crop / luma as basicsr.metrics forms it -- int64
    (exact) for image_range 255 without luma, float64 otherwise; ``ssim_sums`` (B, C') float64 holds the sum of the SSIM map per scored
    channel (C' = 1 for luma), or None with ``ssim=False``."""
    lib = _lib.load()
    (img, img2), dims, cp = _msmetric_args("image_metric_sums", "calculate_psnr / calculate_ssim", (img, img2), crop_border, test_y_channel,
                                           image_range, _METRIC_SSIM if ssim else 0,
                                           "expected two (B, C, H, W) tensors of one shape, got {0[0]} and {0[1]}")
    B, dev = dims[0], img.device
    luma = cp != dims[1]
    sse = torch.empty(B, dtype=torch.int64 if (image_range == 255 and not luma) else torch.float64, device=dev)
    sums = torch.empty(B, cp, dtype=torch.float64, device=dev) if ssim else None
    nws = lib.dcpt_imgmetric_ws_bytes(*dims)   # (0 for arguments the entry point refuses: it then names the reason)
    ws = _workspace(dev, nws)
    _call(lib.dcpt_imgmetric, (img, img2, sse, sums, ws, nws), dims, dev)   # (irregular: the queried size, not the buffer's)
    return sse, sums


# ------------------------------------------------------------------------------------------------
# MS-SSIM, MATLAB SSIM and the NRMSE range (include/dcpt_hip.h dcpt_msssim, dcpt_ssim_matlab, dcpt_imgrange; dcpt_amd/csrc/metrics_ms.hip):
# the sums basicsr.metrics finishes on the host, no autograd, no host sync.
MSMETRIC_TILE = METRIC_TILE   # (TH, TW) of metrics_ms.hip: map positions (MS-SSIM) / output pixels (MATLAB SSIM) per workgroup
MSSSIM_MAX_LEVELS = 8         # MSSSIM_MAX_LEVELS of dcpt_amd/csrc/kernels.h
RANGE_CHUNK = 4096            # METRIC_RANGE_CHUNK: scored values per workgroup of the range kernel


def _scored_channels(channels, test_y_channel):
    """C': the luma of an RGB image is one channel"""
    return 1 if (test_y_channel and channels == 3) else channels


def _msmetric_args(name, host_name, imgs, crop_border, test_y_channel, image_range, more_flags=0, mismatch="expected (B, C, H, W) tensors of one shape, got {}"):
    """the checks every metric op makes before the call; returns the contiguous tensors, the geometry (B, C, H, W, crop, flags) and C'.
    ``mismatch``: the wording of the shape error, formatted with the list of shapes"""
    # (plain comparisons, no generator or loop over the one or two images: this runs once per validation image, in front of a ~0.1 ms launch)
    img, img2 = imgs[0], imgs[-1]   # (``imgs`` holds one or two images: for the one-image op img2 is img itself and its checks repeat img's)
    if not (torch.is_tensor(img) and torch.is_tensor(img2)):
        raise _lib.DcptHipError(f"{name} takes device tensors (got {type(img).__name__}); host arrays go to basicsr.metrics.{host_name}")
    _require_gpu(*imgs)
    if img.dim() != 4 or img2.shape != img.shape:
        raise ValueError(mismatch.format([tuple(t.shape) for t in imgs]))
    if image_range not in (255, 1):
        raise ValueError(f"image_range {image_range}: the device metrics know 255 and 1")
    B, Cc, H, W = img.shape
    img = _contig(img.detach())
    imgs = (img, _contig(img2.detach())) if len(imgs) == 2 else (img,)
    flags = (_METRIC_Y if test_y_channel else 0) | (_METRIC_RANGE1 if image_range == 1 else 0) | more_flags
    return imgs, (B, Cc, H, W, int(crop_border), flags), _scored_channels(Cc, test_y_channel)


def msssim_sums(img, img2, crop_border=0, test_y_channel=False, image_range=255, levels=5):
    """``img`` / ``img2`` as for ``image_metric_sums``.  Returns the float64 device tensor (B, levels, 2): for evaluation k of the reference's
    ``calculate_msssim`` the sums of the SSIM map and of the CS map over the (H' - 10) (W' - 10) positions of channel k mod C' after k box
    blurs.  One launch for all levels plus one reduce; nothing is synchronised."""
    lib = _lib.load()
    (img, img2), dims, _ = _msmetric_args("msssim_sums", "calculate_msssim", (img, img2), crop_border, test_y_channel, image_range)
    levels = int(levels)
    out = torch.empty(dims[0], min(max(levels, 1), MSSSIM_MAX_LEVELS), 2, dtype=torch.float64, device=img.device)   # (a refused count never launches)
    nws = lib.dcpt_msssim_ws_bytes(*dims, levels)   # (0 for arguments the entry point refuses: it then names the reason)
    ws = _workspace(img.device, nws)
    _call(lib.dcpt_msssim, (img, img2, out, ws, nws), (*dims, levels), img.device)   # (irregular: the queried size, not the buffer's)
    return out


def ssim_matlab_sums(img, img2, crop_border=0, test_y_channel=False, image_range=255):
    """Returns the float64 device tensor (B, C'): the sum of the reference's ``calculate_ssim_matlab`` map (the 11 x 11 Gaussian window at
    every pixel under replicate padding) over the H' W' pixels of each scored channel.  Nothing is synchronised."""
    lib = _lib.load()
    (img, img2), dims, cp = _msmetric_args("ssim_matlab_sums", "calculate_ssim_matlab", (img, img2), crop_border, test_y_channel, image_range)
    out = torch.empty(dims[0], cp, dtype=torch.float64, device=img.device)
    nws = lib.dcpt_ssim_matlab_ws_bytes(*dims)
    ws = _workspace(img.device, nws)
    _call(lib.dcpt_ssim_matlab, (img, img2, out, ws, nws), dims, img.device)
    return out


def image_range_minmax(img, crop_border=0, test_y_channel=False, image_range=255):
    """Returns the float64 device tensor (B, 2): the minimum and the maximum of each image's scored values (after quantisation / crop / luma),
    what the reference's ``calculate_nrmse`` divides by.  Nothing is synchronised."""
    lib = _lib.load()
    (img,), dims, _ = _msmetric_args("image_range_minmax", "calculate_nrmse", (img,), crop_border, test_y_channel, image_range)
    out = torch.empty(dims[0], 2, dtype=torch.float64, device=img.device)
    nws = lib.dcpt_imgrange_ws_bytes(*dims)
    ws = _workspace(img.device, nws)
    _call(lib.dcpt_imgrange, (img, out, ws, nws), dims, img.device)
    return out


# ------------------------------------------------------------------------------------------------
# SSIM as a training loss (include/dcpt_hip.h dcpt_ssim_loss_fwd / _bwd): the reference's calculate_ssim_pt with its gradient, in fp64 on
# the device, without its grouped fp64 convolutions.
def ssim_plane_cap(nbytes=None):
    """bytes of fp64 planes the backward pass of ``ssim_pt`` holds at a time (the batch goes through in chunks of whole images, at least
    one): returns the value, sets it first if ``nbytes`` is given.  The tests shrink it to drive the chunk loop with small images."""
    cap = C.c_size_t.in_dll(_lib.load(), "dcpt_ssim_loss_plane_cap")
    if nbytes is not None:
        cap.value = int(nbytes)
    return int(cap.value)


def _ssim_geom(pred, crop_border, test_y_channel):
    B, Cc, H, W = pred.shape
    crop = int(crop_border)
    cp = _scored_channels(Cc, test_y_channel)
    return (B, Cc, H, W, crop, _METRIC_Y if test_y_channel else 0), cp, cp * (H - 2 * crop - 10) * (W - 2 * crop - 10)


class _SsimPtFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, crop_border, test_y_channel, image_range):
        lib = _lib.load()
        pred, target = _contig(pred), _contig(target)
        dev = pred.device
        dims, cp, count = _ssim_geom(pred, crop_border, test_y_channel)
        sums = torch.empty(dims[0], cp, dtype=torch.float64, device=dev)
        nws = lib.dcpt_ssim_loss_ws_bytes(*dims, 0)   # (0 for arguments the entry point refuses: it then names the reason)
        ws = _workspace(dev, nws)
        _call(lib.dcpt_ssim_loss_fwd, (pred, target, sums, ws, nws), (*dims, float(image_range)), dev)   # (irregular: the queried size)
        ctx.save_for_backward(pred, target)
        ctx.args = (crop_border, test_y_channel, float(image_range))
        return sums.sum(1) / count

    @staticmethod
    def backward(ctx, dssim):
        lib = _lib.load()
        pred, target = ctx.saved_tensors
        crop_border, test_y_channel, image_range = ctx.args
        dev = pred.device
        dims, cp, count = _ssim_geom(pred, crop_border, test_y_channel)
        gscale = _contig((dssim.to(torch.float64) / count).reshape(-1, 1).expand(-1, cp))
        dpred = torch.empty_like(pred)
        nws = lib.dcpt_ssim_loss_ws_bytes(*dims, 1)
        ws = _workspace(dev, nws)
        _call(lib.dcpt_ssim_loss_bwd, (pred, target, gscale, dpred, ws, nws), (*dims, image_range), dev)
        return dpred, None, None, None, None


def ssim_pt(pred, target, crop_border=0, test_y_channel=False, image_range=1.0):
    """The reference's ``calculate_ssim_pt`` (basicsr/metrics/psnr_ssim.py:436-480): ``pred`` / ``target`` (B, C, H, W) fp32 device tensors,
    C in {1, 3}; returns the per-image SSIM as a float64 tensor (B,), differentiable with respect to ``pred`` (fp32 gradient, rounded once
    from fp64).  ``target`` gets no gradient: one that requires it is refused."""
    if not (torch.is_tensor(pred) and torch.is_tensor(target)):
        raise _lib.DcptHipError(f"ssim_pt takes device tensors (got {type(pred).__name__}, {type(target).__name__})")
    _require_gpu(pred, target)
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"expected two (B, C, H, W) tensors of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if target.requires_grad:
        raise NotImplementedError("ssim_pt differentiates with respect to pred only; detach the target")
    return _SsimPtFn.apply(pred, target, int(crop_border), bool(test_y_channel), image_range)


# ------------------------------------------------------------------------------------------------
# The LDL artifact-weight map (include/dcpt_hip.h dcpt_ldl_weight_fwd / _bwd): the reference's get_refined_artifact_map(std=True) with its
# gradient, in fp64 on the device, without the 49-fold unfold of the residual.
class _LdlWeightFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt, out):
        lib = _lib.load()
        gt, out = _contig(gt), _contig(out)
        dev = out.device
        dims = tuple(out.shape)
        w = torch.empty_like(out)
        if ctx.needs_input_grad[1]:
            # the backward reads what the forward leaves (m, s, the planes u and mu): a buffer of this call's own, of the backward's size
            nws = lib.dcpt_ldl_weight_ws_bytes(*dims, 1)   # (0 for a shape the entry point refuses: it then names the reason)
            ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
            ctx.save_for_backward(gt, out, ws)
        else:
            nws = lib.dcpt_ldl_weight_ws_bytes(*dims, 0)
            ws = _workspace(dev, nws)
        _call(lib.dcpt_ldl_weight_fwd, (gt, out, w, ws, nws), dims, dev)   # (irregular: the queried size, not the buffer's)
        return w

    @staticmethod
    def backward(ctx, gw):
        lib = _lib.load()
        gt, out, ws = ctx.saved_tensors
        dout = torch.empty_like(out)
        _call(lib.dcpt_ldl_weight_bwd, (gt, out, _contig(gw.float()), dout, ws, ws.numel()), tuple(out.shape), out.device)
        return None, dout


def ldl_weight(gt, out):
    """The reference's ``get_refined_artifact_map(gt, out, std=True)`` (basicsr/losses/loss_util.py:100-165, window 7, no ``img_ema``):
    ``gt`` / ``out`` (B, C, H, W) fp32 device tensors, H, W >= 4; returns the weight map w = (tanh((u - mean u) / std u) + 1) / 2 of the local
    7 x 7 standard deviation u of |gt - out| as an fp32 tensor of the same shape, differentiable with respect to ``out`` (the map is not
    detached in the reference either; fp32 gradient, rounded once from fp64).  ``gt`` gets no gradient: one that requires it is refused."""
    if not (torch.is_tensor(gt) and torch.is_tensor(out)):
        raise _lib.DcptHipError(f"ldl_weight takes device tensors (got {type(gt).__name__}, {type(out).__name__})")
    _require_gpu(gt, out)
    if out.dim() != 4 or out.shape != gt.shape:
        raise ValueError(f"expected two (B, C, H, W) tensors of one shape, got {tuple(gt.shape)} and {tuple(out.shape)}")
    if gt.requires_grad:
        raise NotImplementedError("ldl_weight differentiates with respect to out only; detach the target")
    return _LdlWeightFn.apply(gt, out)


# ------------------------------------------------------------------------------------------------
# The DiffJPEG round trip (include/dcpt_hip.h dcpt_diffjpeg_fwd): the reference's DiffJPEG.forward (basicsr/utils/diffjpeg.py:494-523) as one
# fp64 kernel, one read and one write of the batch.
JPEG_DIFF_ROUND, JPEG_UINT8_IO = 1, 2   # include/dcpt_hip.h DCPT_JPEG_*


def diffjpeg(x, quality, differentiable=False, uint8_io=False):
    """The JPEG round trip of ``DiffJPEG(differentiable).forward(x, quality)``: ``x`` (B, 1 or 3, H, W) fp32 device tensor in [0, 1] (any
    strides: it is made contiguous NCHW); ``quality`` a Python number in (0, 100) -- at 100 the reference's factor is 0 and it divides by
    zero -- or a (B,) tensor with one quality per image.  Returns the decoded batch, fp32 NCHW.  ``differentiable=True`` runs the
    reference's cubic ``diff_round`` in the FORWARD; there is no backward pass (an input that requires grad raises under grad mode).
    ``uint8_io=True``: the input is first rounded to the 8-bit grid and the output is ``rint(decoded) / 255``, what the reference's dataset
    gets from ``cv2.imencode`` / ``imdecode`` (paired_image_dataset.py:539-546).  One departure from the reference: the caller's quality
    tensor is NOT modified (the reference overwrites it in place with the factors, diffjpeg.py:504-505)."""
    if not torch.is_tensor(x):
        raise _lib.DcptHipError(f"diffjpeg takes a device tensor (got {type(x).__name__})")
    _require_gpu(x)
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise ValueError(f"diffjpeg: expected a (B, 1 or 3, H, W) batch, got {tuple(x.shape)}")
    _inference_only("diffjpeg", x, what="the JPEG round trip")
    B, C, H, W = x.shape
    dev = x.device
    if torch.is_tensor(quality):
        if quality.numel() != B or quality.dim() > 1:
            raise ValueError(f"diffjpeg: quality must be a number or a ({B},) tensor, got {tuple(quality.shape)}")
        q = quality.detach().to(device=dev, dtype=torch.float32).reshape(B).contiguous()   # (read by the kernel, never written)
    else:
        if not 0 < float(quality) < 100:
            raise ValueError(f"diffjpeg: quality must lie in (0, 100), got {quality!r} (at 100 the quantisation factor is 0)")
        q = torch.full((B,), float(quality), dtype=torch.float32, device=dev)
    x = x.detach().contiguous()
    y = torch.empty_like(x)
    flags = (JPEG_DIFF_ROUND if differentiable else 0) | (JPEG_UINT8_IO if uint8_io else 0)
    _call(_lib.load().dcpt_diffjpeg_fwd, (x, q, y), (B, C, H, W, flags), dev)
    return y


# ------------------------------------------------------------------------------------------------
# The demosaic and the line-mask inpainting degradation (include/dcpt_hip.h dcpt_demosaic_fwd, dcpt_inpaint_lines_fwd): lq from gt in one
# launch each, one read and one write of the batch.
DEMOSAIC_BILINEAR, DEMOSAIC_UINT8_IO = 1, 2   # include/dcpt_hip.h DCPT_DEMOSAIC_*
DEMOSAIC_METHODS = ("malvar", "bilinear")     # the index is the int a ``demosaic_backend: device`` sample carries in ``mosaic``
INPAINT_MAX_LINES, INPAINT_MAX_THICK, INPAINT_MAX_COORD = 10, 64, 16384


def demosaic(x, method="malvar", uint8_io=False):
    """Bayer demosaic of a batch: ``x`` (B, 3, H, W) an RGB image, mosaicked (RGGB) inside the kernel, or (B, 1, H, W) the CFA plane
    itself; fp32 device tensor (any strides: it is made contiguous NCHW), H and W at least 3, odd sizes allowed.  Returns (B, 3, H, W).
    ``method="malvar"``: Malvar-He-Cutler with reflect padding, the reference's ``dm_matlab``; ``"bilinear"``: its ``dm`` (circular
    padding).  ``uint8_io=False``: fp32 sums of the raw input, what the reference's functions return.  ``uint8_io=True``: the input is put
    on the 8-bit grid, the taps are summed in integers and the output is ``rint(clamp(S / 16, 0, 255)) / 255``.  Forward only."""
    if not torch.is_tensor(x):
        raise _lib.DcptHipError(f"demosaic takes a device tensor (got {type(x).__name__})")
    _require_gpu(x)
    if x.dim() != 4 or x.shape[1] not in (1, 3) or x.shape[0] < 1 or x.shape[2] < 3 or x.shape[3] < 3:
        raise ValueError(f"demosaic: expected a (B, 1 or 3, H >= 3, W >= 3) batch, got {tuple(x.shape)}")
    if method not in DEMOSAIC_METHODS:
        raise ValueError(f"demosaic: method must be one of {DEMOSAIC_METHODS}, got {method!r}")
    _inference_only("demosaic", x, what="the demosaic")
    B, C, H, W = x.shape
    x = x.detach().contiguous()
    y = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
    flags = (DEMOSAIC_BILINEAR if method == "bilinear" else 0) | (DEMOSAIC_UINT8_IO if uint8_io else 0)
    _call(_lib.load().dcpt_demosaic_fwd, (x, y), (B, C, H, W, flags), x.device)
    return y


def inpaint_lines(x, lines, meta):
    """The inpainting degradation: ``x`` (B, 1 or 3, H, W) fp32 device tensor; ``lines`` (B, 10, 4) integers ``x1, y1, x2, y2`` per stroke;
    ``meta`` (B, 3) integers ``n_lines, thick, white``.  A pixel within ``thick / 2`` of one of the first ``n_lines`` segments becomes 1
    (``white``) or 0 in every channel, any other ``clamp(x, 0, 1)``.  ``lines`` / ``meta`` on the host are validated here (``n_lines`` in
    0..10, ``thick`` in 1..64, coordinates in -16384..16384) and copied to the device; device tensors are not read back, and the kernel
    clamps them to those ranges.  Returns a new tensor.  Forward only."""
    if not torch.is_tensor(x):
        raise _lib.DcptHipError(f"inpaint_lines takes a device tensor (got {type(x).__name__})")
    _require_gpu(x)
    if x.dim() != 4 or x.shape[1] not in (1, 3) or 0 in x.shape or x.shape[2] > INPAINT_MAX_COORD or x.shape[3] > INPAINT_MAX_COORD:
        raise ValueError(f"inpaint_lines: expected a (B, 1 or 3, H, W) batch with H, W <= {INPAINT_MAX_COORD}, got {tuple(x.shape)}")
    B, C, H, W = x.shape
    if not torch.is_tensor(lines) or not torch.is_tensor(meta) or lines.is_floating_point() or meta.is_floating_point():
        raise ValueError("inpaint_lines: lines and meta must be integer tensors")
    if tuple(lines.shape) != (B, INPAINT_MAX_LINES, 4) or tuple(meta.shape) != (B, 3):
        raise ValueError(f"inpaint_lines: expected lines ({B}, {INPAINT_MAX_LINES}, 4) and meta ({B}, 3), got {tuple(lines.shape)} and "
                         f"{tuple(meta.shape)}")
    if not meta.is_cuda:
        if bool(((meta[:, 0] < 0) | (meta[:, 0] > INPAINT_MAX_LINES)).any()):
            raise ValueError(f"inpaint_lines: n_lines must lie in 0..{INPAINT_MAX_LINES}, got {meta[:, 0].tolist()}")
        if bool(((meta[:, 1] < 1) | (meta[:, 1] > INPAINT_MAX_THICK)).any()):
            raise ValueError(f"inpaint_lines: thick must lie in 1..{INPAINT_MAX_THICK}, got {meta[:, 1].tolist()}")
    if not lines.is_cuda and bool((lines.abs() > INPAINT_MAX_COORD).any()):
        raise ValueError(f"inpaint_lines: an endpoint lies outside -{INPAINT_MAX_COORD}..{INPAINT_MAX_COORD}")
    _inference_only("inpaint_lines", x, what="the inpainting degradation")
    dev = x.device
    lines = lines.to(device=dev, dtype=torch.int32).contiguous()
    meta = meta.to(device=dev, dtype=torch.int32).contiguous()
    x = x.detach().contiguous()
    y = torch.empty_like(x)
    _call(_lib.load().dcpt_inpaint_lines_fwd, (x, lines, meta, y), (B, C, H, W), dev)
    return y


# ------------------------------------------------------------------------------------------------
# Gaussian noise from a per-image Philox4x32-10 stream (include/dcpt_hip.h dcpt_gauss_noise_fwd): lq from gt in one launch.
NOISE_CLIP, NOISE_ROUND8, NOISE_ONLY = 1, 2, 4   # include/dcpt_hip.h DCPT_NOISE_*
NOISE_MAX_ELEMS = 1 << 34                        # C * H * W of one image stays below this


def _per_image(name, v, B, dtype, dev, op="gaussian_noise"):
    """a per-image argument as a (B,) device tensor: a Python number for every image, or a tensor of B values (0-d or one value: for every
    image); a device tensor is never read back"""
    if torch.is_tensor(v):
        if v.numel() not in (1, B) or v.dim() > 1 and v.numel() != B:
            raise ValueError(f"{op}: {name} must be a number or hold {B} values, got {tuple(v.shape)}")
        v = v.detach().reshape(-1).to(device=dev, dtype=dtype, non_blocking=True)
        return (v.expand(B) if v.numel() != B else v).contiguous()
    return torch.full((B,), v, dtype=dtype, device=dev)


def gaussian_noise(x, sigma, key, gray=None, clip=False, rounds=False, noise_only=False, out=None):
    """``x + sigma / 255 * n`` with n standard normal: ``x`` (B, C, H, W) fp32 device tensor (any strides: it is made contiguous NCHW),
    ``sigma`` the standard deviation on the 0..255 scale, ``key`` the 64-bit key of the image's Philox4x32-10 stream (include/dcpt_hip.h
    states the generator), ``gray`` non-zero for one noise plane shared by the channels.  ``sigma``, ``key`` and ``gray`` are Python
    numbers (for every image: one key gives every image the same noise) or tensors of B values, on the host or the device; a device
    tensor is not read back, so only a host sigma is checked (a negative one raises).  The sum is taken in fp64 and rounded once;
    ``sigma == 0`` without flags returns ``x`` bit for bit.  ``clip``: clamp to [0, 1]; ``rounds``: ``rint(255 v) / 255`` after it;
    ``noise_only``: the noise term without ``x`` (``x`` then gives the shape and the device only).  ``out``: a contiguous fp32 tensor
    of x's shape on its device to write into; ``out=x`` works in place.  An image's result depends on its own values only, not on the
    batch around it.  Forward only."""
    x, sigma, key, gray, out, flags = _noise_args("gaussian_noise", x, "sigma", sigma, key, gray, clip, rounds, noise_only, out)
    _call(_lib.load().dcpt_gauss_noise_fwd, (None if noise_only else x, sigma, key, gray, out), (*x.shape, flags), x.device)
    return out


def _noise_args(op, x, amp_name, amp, key, gray, clip, rounds, noise_only, out):
    """the arguments the two noise ops share, checked and brought to the device: returns (x, amp, key, gray, out, flags)"""
    if not torch.is_tensor(x):
        raise _lib.DcptHipError(f"{op} takes a device tensor (got {type(x).__name__})")
    _require_gpu(x)
    if x.dim() != 4 or 0 in x.shape or x.shape[1] * x.shape[2] * x.shape[3] >= NOISE_MAX_ELEMS:
        raise ValueError(f"{op}: expected a non-empty (B, C, H, W) batch with C * H * W < 2^34, got {tuple(x.shape)}")
    _inference_only(op, x, what="the noise degradation")
    B = x.shape[0]
    dev = x.device
    host_amp = amp if not torch.is_tensor(amp) else (None if amp.is_cuda else amp)
    if host_amp is not None and bool(torch.as_tensor(host_amp).lt(0).any()):
        raise ValueError(f"{op}: {amp_name} must not be negative, got {host_amp!r}")
    if not torch.is_tensor(key):
        key = int(key)
        if not -(1 << 63) <= key < (1 << 64):
            raise ValueError(f"{op}: key must fit 64 bits, got {key}")
        key = key - (1 << 64) if key >= (1 << 63) else key   # (the same 64 bits as a signed value)
    elif key.is_floating_point():
        raise ValueError(f"{op}: key must be an integer tensor")
    amp = _per_image(amp_name, amp if torch.is_tensor(amp) else float(amp), B, torch.float32, dev, op)
    key = _per_image("key", key, B, torch.int64, dev, op)
    if gray is not None:
        gray = _per_image("gray", gray.ne(0) if torch.is_tensor(gray) else int(bool(gray)), B, torch.int32, dev, op)
    x = x.detach().contiguous()   # (no copy of a contiguous x, so out=x stays in place)
    if out is None:
        out = torch.empty_like(x)
    else:
        if not torch.is_tensor(out) or out.shape != x.shape or out.device != dev or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"{op}: out must be a contiguous fp32 tensor of shape {tuple(x.shape)} on {dev}")
        _inference_only(op, out, what="the noise degradation")
    flags = (NOISE_CLIP if clip else 0) | (NOISE_ROUND8 if rounds else 0) | (NOISE_ONLY if noise_only else 0)
    return x, amp, key, gray, out, flags


def poisson_noise(x, scale, key, gray=None, clip=False, rounds=False, noise_only=False, out=None, return_vals=False):
    """Poisson (shot) noise of the reference's ``generate_poisson_noise_pt``: ``x + scale * (Poisson(q vals) / vals - q)`` with ``q`` the
    image on the 8-bit grid and ``vals`` the number of its distinct levels rounded up to a power of two (include/dcpt_hip.h
    dcpt_poisson_noise_fwd states the level count, the Philox stream and the sampler).  Arguments as for ``gaussian_noise``, with ``scale``
    in place of ``sigma``: per-image values are Python numbers or tensors of B values on the host or the device, a device tensor is not read
    back (only a host scale is checked: a negative one raises).  ``gray`` non-zero: the noise is made from the image's gray values, one plane
    shared by the channels; it needs 1 or 3 channels.  ``noise_only`` writes the noise term; ``x`` is read all the same, the rate depends on
    it.  ``scale == 0`` without flags returns ``x`` bit for bit; ``out=x`` works in place.  Two launches: the level count and the sampler.
    ``return_vals=True`` returns ``(out, vals)`` with ``vals`` the int32 (B,) device tensor of the per-image level counts.  Forward only."""
    x, scale, key, gray, out, flags = _noise_args("poisson_noise", x, "scale", scale, key, gray, clip, rounds, noise_only, out)
    B, C, H, W = x.shape
    if gray is not None and C not in (1, 3):
        raise ValueError(f"poisson_noise: gray noise needs 1 or 3 channels, got {C}")
    lib = _lib.load()
    dev = x.device
    nws = _check_ws("poisson_noise", lib.dcpt_poisson_noise_ws_bytes(B, C, H, W), f"B={B} C={C} H={H} W={W}")
    ws = _workspace(dev, nws)
    _call(lib.dcpt_poisson_noise_fwd, (x, scale, key, gray, out, ws, nws), (B, C, H, W, flags), dev)
    if return_vals:
        return out, ws[:4 * B].view(torch.int32).clone()   # (the workspace is reused by the next op of the stream)
    return out


# ------------------------------------------------------------------------------------------------
# Synthetic blur (include/dcpt_hip.h dcpt_filter2d_fwd): the reference's filter2D (basicsr/utils/img_process_util.py:7-31) as one launch,
# without the padded copy of the batch and the weight repeated over the channels.
FILTER2D_MAX_K = 51


def filter2d(x, kernel):
    """The K x K correlation (no flip, as ``F.conv2d``) of every channel of image b with ``kernel[b]`` over the image reflect-padded by
    K // 2: ``x`` (B, C, H, W) fp32 device tensor (any strides: it is made contiguous NCHW); ``kernel`` (B, K, K), or (1, K, K) for one
    kernel shared by the batch, any float dtype on any device (it is copied to fp32 on x's device); K odd, 1..51, K // 2 < H and W.
    Returns a new fp32 NCHW tensor.  Each output is one fp64 sum over the taps, rows outer and columns inner, rounded once to fp32
    (the header states it; ``basicsr.data.filter2d_host`` gives the same bits on the host).  Forward only."""
    if not torch.is_tensor(x):
        raise _lib.DcptHipError(f"filter2d takes a device tensor (got {type(x).__name__})")
    _require_gpu(x)
    if x.dim() != 4 or 0 in x.shape:
        raise ValueError(f"filter2d: expected a non-empty (B, C, H, W) batch, got {tuple(x.shape)}")
    B, C, H, W = x.shape
    if not torch.is_tensor(kernel) or not kernel.is_floating_point() or kernel.dim() != 3 or kernel.shape[1] != kernel.shape[2] \
            or kernel.shape[0] not in (1, B):
        raise ValueError(f"filter2d: kernel must be a float ({B}, K, K) or (1, K, K) tensor, got "
                         f"{tuple(kernel.shape) if torch.is_tensor(kernel) else type(kernel).__name__}")
    K = kernel.shape[-1]
    if K % 2 == 0 or not 1 <= K <= FILTER2D_MAX_K:
        raise ValueError(f"filter2d: K must be odd and lie in 1..{FILTER2D_MAX_K}, got a kernel of {tuple(kernel.shape)}")
    if K // 2 >= H or K // 2 >= W:
        raise ValueError(f"filter2d: the reflect padding K // 2 = {K // 2} must be smaller than H and W, got x {tuple(x.shape)} and a "
                         f"kernel of {tuple(kernel.shape)}")
    _inference_only("filter2d", x, kernel, what="the blur")
    dev = x.device
    kernel = kernel.detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
    x = x.detach().contiguous()
    y = torch.empty_like(x)
    _call(_lib.load().dcpt_filter2d_fwd, (x, kernel, y), (B, C, H, W, K, int(kernel.shape[0] != 1)), dev)
    return y


# ------------------------------------------------------------------------------------------------
# The resize of the second-order degradation chain (include/dcpt_hip.h dcpt_interp_fwd): F.interpolate's area / bilinear / bicubic modes
# with align_corners=False as one launch, taps and sums in fp64.
INTERP_MODES = ("area", "bilinear", "bicubic")   # the index is the mode of the C ABI (DCPT_INTERP_*)
INTERP_CLIP, INTERP_ROUND8 = 1, 2                # include/dcpt_hip.h DCPT_INTERP_*
INTERP_MAX_PLANE = 1 << 30


def interp_geometry(in_size, size=None, scale_factor=None):
    """torch's rules for the output size and the source-per-destination ratios of ``F.interpolate`` (align_corners=False,
    recompute_scale_factor unset): with ``scale_factor`` (a number or a pair) ``Ho = floor(H * sf)`` in double and ``ratio = 1 / sf``; with
    ``size`` (an int or a pair) ``ratio = H / Ho``.  Returns ``((Ho, Wo), (ratio_h, ratio_w))``; needs no device."""
    if (size is None) == (scale_factor is None):
        raise ValueError("interpolate: exactly one of size and scale_factor must be given")
    H, W = (int(v) for v in in_size)
    if scale_factor is not None:
        sf = tuple(scale_factor) if isinstance(scale_factor, (tuple, list)) else (scale_factor, scale_factor)
        if len(sf) != 2 or not all(isinstance(v, (int, float)) and math.isfinite(v) and v > 0 for v in sf):
            raise ValueError(f"interpolate: scale_factor must be a positive number or a pair of them, got {scale_factor!r}")
        out = (int(math.floor(float(H * sf[0]))), int(math.floor(float(W * sf[1]))))
        ratio = (1.0 / sf[0], 1.0 / sf[1])
    else:
        out = tuple(size) if isinstance(size, (tuple, list)) else (size, size)
        if len(out) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in out):
            raise ValueError(f"interpolate: size must be an int or a pair of ints, got {size!r}")
        ratio = (H / out[0] if out[0] > 0 else 0.0, W / out[1] if out[1] > 0 else 0.0)
    if min(out) < 1:
        raise ValueError(f"interpolate: the output size must be positive, got {out} from an input of {(H, W)}")
    return out, ratio


def interpolate(x, size=None, scale_factor=None, mode="bilinear", clip=False, rounds=False):
    """``F.interpolate(x, size, scale_factor, mode, align_corners=False)`` for ``mode`` ``"area"``, ``"bilinear"`` or ``"bicubic"``: ``x``
    (B, C, H, W) fp32 device tensor (any strides: it is made contiguous NCHW); exactly one of ``size`` (an int or a pair) and
    ``scale_factor`` (a number or a pair) with torch's rules for the output size and the ratios (``interp_geometry``).  The taps and both
    sums are fp64 and an output is rounded once (include/dcpt_hip.h states the arithmetic), so the result is within one fp32 rounding of
    torch's float64 result.  ``clip``: clamp to [0, 1]; ``rounds``: ``rint(255 v) / 255`` after it.  Returns a new fp32 NCHW tensor; one
    launch, nothing is read back.  Forward only; ``align_corners=True``, ``nearest`` and antialiasing are not offered."""
    if not torch.is_tensor(x):
        raise _lib.DcptHipError(f"interpolate takes a device tensor (got {type(x).__name__})")
    _require_gpu(x)
    if x.dim() != 4 or 0 in x.shape:
        raise ValueError(f"interpolate: expected a non-empty (B, C, H, W) batch, got {tuple(x.shape)}")
    if mode not in INTERP_MODES:
        raise ValueError(f"interpolate: mode must be one of {INTERP_MODES}, got {mode!r}")
    B, C, H, W = x.shape
    (Ho, Wo), (rh, rw) = interp_geometry((H, W), size, scale_factor)
    if H * W > INTERP_MAX_PLANE or Ho * Wo > INTERP_MAX_PLANE:
        raise ValueError(f"interpolate: a plane above 2^30 pixels ({(H, W)} -> {(Ho, Wo)})")
    _inference_only("interpolate", x, what="the resize")
    x = x.detach().contiguous()
    y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
    flags = (INTERP_CLIP if clip else 0) | (INTERP_ROUND8 if rounds else 0)
    _call(_lib.load().dcpt_interp_fwd, (x, y), (B, C, H, W, Ho, Wo, INTERP_MODES.index(mode), rh, rw, flags), x.device)
    return y


# ------------------------------------------------------------------------------------------------
# The kNN degradation probe (include/dcpt_hip.h dcpt_pdist2_fwd, dcpt_knn_vote_fwd): fp64 squared distances between flattened feature rows
# on the fp64 matrix cores, and the k-nearest-neighbour majority vote over them.  Forward only.
PDIST_BF16 = 1                           # include/dcpt_hip.h DCPT_PDIST_BF16
PDIST_MAX_ROWS, KNN_MAX_K = 65535, 32


def _feature_rows(op, name, x):
    if not torch.is_tensor(x):
        raise _lib.DcptHipError(f"{op} takes device tensors (got {type(x).__name__} for {name})")
    _require_gpu_feat(x)
    if x.dim() != 2 or 0 in x.shape or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise ValueError(f"{op}: {name} must be a non-empty 2-D tensor with contiguous rows, got shape {tuple(x.shape)} strides {x.stride()}")
    return x.detach()


def pairwise_sqdist(xq, xt=None, ksplit=0, out=None):
    """Squared Euclidean distances between the rows of ``xq`` (Nq, D) and ``xt`` (Nt, D; None: ``xq`` itself) as a float64 (Nq, Nt) device
    tensor.  The operands are fp32 or bf16 device tensors of one dtype whose rows are contiguous; any row stride of at least D is allowed.
    Every element is converted to fp64 and ``max(0, (|q|^2 + |t|^2) - 2 q.t)`` is summed in fp64 on the fp64 matrix cores, the k-range in
    ``ksplit`` chunks (0: chosen from the shape); an entry depends on its two rows, D, the dtype and the effective ``ksplit`` only, so two
    runs and permuted rows give the same bits (include/dcpt_hip.h states the arithmetic).  ``out``: a float64 (Nq, Nt) device tensor with
    contiguous rows to write into.  Forward only."""
    xq = _feature_rows("pairwise_sqdist", "xq", xq)
    xt = xq if xt is None else _feature_rows("pairwise_sqdist", "xt", xt)
    if xt.dtype != xq.dtype or xt.device != xq.device or xt.shape[1] != xq.shape[1]:
        raise ValueError(f"pairwise_sqdist: xq {tuple(xq.shape)} {xq.dtype} on {xq.device} and xt {tuple(xt.shape)} {xt.dtype} on {xt.device} "
                         "must share the dtype, the device and the row length")
    (Nq, D), Nt, dev = xq.shape, xt.shape[0], xq.device
    ksplit = int(ksplit)
    if max(Nq, Nt) > PDIST_MAX_ROWS or not 0 <= ksplit <= min((D + 3) // 4, 65535):
        raise ValueError(f"pairwise_sqdist: at most {PDIST_MAX_ROWS} rows and ksplit in 0 .. min(ceil(D / 4), 65535), got Nq={Nq} Nt={Nt} D={D} "
                         f"ksplit={ksplit}")
    if out is None:
        out = torch.empty((Nq, Nt), dtype=torch.float64, device=dev)
    elif not torch.is_tensor(out) or tuple(out.shape) != (Nq, Nt) or out.dtype != torch.float64 or out.device != dev or out.stride(1) != 1 \
            or (Nq > 1 and out.stride(0) < Nt):
        raise ValueError(f"pairwise_sqdist: out must be a float64 ({Nq}, {Nt}) tensor with contiguous rows on {dev}")
    lib = _lib.load()
    nws = _check_ws("pairwise_sqdist", lib.dcpt_pdist2_ws_bytes(Nq, Nt, D, ksplit), f"Nq={Nq} Nt={Nt} D={D} ksplit={ksplit}")
    ws = _workspace(dev, nws)
    ldq, ldt, ldd = (t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in (xq, xt, out))
    _call(lib.dcpt_pdist2_fwd, (xq, xt, out, ws, nws), (Nq, Nt, D, ldq, ldt, ldd, ksplit, PDIST_BF16 if xq.dtype == torch.bfloat16 else 0), dev)
    return out


def _index_lists(name, v, bound, dev):
    """an (S, n) index argument as a contiguous int32 device tensor; a host tensor or nested list is checked against 0 .. bound - 1"""
    if not torch.is_tensor(v):
        v = torch.as_tensor(v)
    if v.is_floating_point() or v.dtype == torch.bool or v.dim() != 2 or 0 in v.shape:
        raise ValueError(f"knn_vote: {name} must be a non-empty (S, n) integer tensor or nested list, got {tuple(v.shape)} {v.dtype}")
    if not v.is_cuda and (int(v.min()) < 0 or int(v.max()) >= bound):
        raise ValueError(f"knn_vote: {name} holds an index outside 0 .. {bound - 1}")
    return v.detach().to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()


def knn_vote(d2, labels, train_idx, test_idx, k):
    """The k nearest training columns of every query row of ``d2`` and their majority label, for S splits in one launch.  ``d2``: float64
    (Nq, Nt) device tensor with contiguous rows; ``labels``: Nt integer labels of d2's columns (any int32 value; tensor or list);
    ``train_idx`` (S, nt) the columns and ``test_idx`` (S, nq) the rows that split s uses: integer tensors or nested lists; host values
    are checked against d2's shape and copied, device tensors are not read back.  Returns ``(pred, nbr, nbr_d2)``: int32 (S, nq), int32
    (S, nq, k) positions in the split's ``train_idx`` nearest first, and their float64 distances.  Neighbours are ordered by (distance,
    position) -- equal distances go to the lower position, a NaN after every number; on equal counts the smallest label wins.  Nothing
    is read back from the device."""
    if not torch.is_tensor(d2):
        raise _lib.DcptHipError(f"knn_vote takes a device tensor (got {type(d2).__name__})")
    _require((d2,), (torch.float64,), "knn_vote: d2 must be float64 (got {})")
    if d2.dim() != 2 or 0 in d2.shape or d2.stride(1) != 1 or (d2.shape[0] > 1 and d2.stride(0) < d2.shape[1]):
        raise ValueError(f"knn_vote: d2 must be a non-empty 2-D tensor with contiguous rows, got {tuple(d2.shape)} strides {d2.stride()}")
    dev = d2.device
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(labels)
    if labels.is_floating_point() or labels.dim() != 1 or labels.numel() != d2.shape[1]:
        raise ValueError(f"knn_vote: labels must be {d2.shape[1]} integers, one per column of d2, got {tuple(labels.shape)} {labels.dtype}")
    labels = labels.detach().to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    t_idx = _index_lists("train_idx", train_idx, d2.shape[1], dev)
    q_idx = _index_lists("test_idx", test_idx, d2.shape[0], dev)
    (S, nt), nq, k = t_idx.shape, q_idx.shape[1], int(k)
    if q_idx.shape[0] != S:
        raise ValueError(f"knn_vote: train_idx has {S} splits and test_idx {q_idx.shape[0]}")
    if not 1 <= k <= min(KNN_MAX_K, nt):
        raise ValueError(f"knn_vote: k must lie in 1 .. min({KNN_MAX_K}, nt = {nt}), got {k}")
    d2 = d2.detach()
    nbr = torch.empty((S, nq, k), dtype=torch.int32, device=dev)
    nbr_d2 = torch.empty((S, nq, k), dtype=torch.float64, device=dev)
    pred = torch.empty((S, nq), dtype=torch.int32, device=dev)
    ldd = d2.stride(0) if d2.shape[0] > 1 else d2.shape[1]
    _call(_lib.load().dcpt_knn_vote_fwd, (d2, ldd, q_idx, t_idx, labels), (S, nq, nt, k, nbr.data_ptr(), nbr_d2.data_ptr(), pred.data_ptr()), dev)
    return pred, nbr, nbr_d2


# ------------------------------------------------------------------------------------------------
# Exact t-SNE on the probe's distance matrix (include/dcpt_hip.h dcpt_tsne_affinity_fwd, dcpt_tsne_joint_fwd, dcpt_tsne_steps_fwd,
# dcpt_tsne_kl_fwd): scikit-learn's method="exact" rules in fp64, two output dimensions.  Forward only.
TSNE_MAX_ROWS = 65535


def _tsne_matrix(op, name, m, N=None):
    """a float64 (N, N) device tensor with contiguous rows -> (detached tensor, leading dimension)"""
    if not torch.is_tensor(m):
        raise _lib.DcptHipError(f"{op} takes device tensors (got {type(m).__name__} for {name})")
    _require((m,), (torch.float64,), op + ": " + name + " must be float64 (got {})")
    if m.dim() != 2 or m.shape[0] != m.shape[1] or m.stride(1) != 1 or m.stride(0) < m.shape[1] or (N is not None and m.shape[0] != N):
        raise ValueError(f"{op}: {name} must be a square 2-D tensor with contiguous rows" + (f" of {N} rows" if N is not None else "")
                         + f", got shape {tuple(m.shape)} strides {m.stride()}")
    if not 2 <= m.shape[0] <= TSNE_MAX_ROWS:
        raise ValueError(f"{op}: N must lie in 2 .. {TSNE_MAX_ROWS}, got {m.shape[0]}")
    return m.detach(), m.stride(0)


def _tsne_points(op, name, y, N, dev):
    """a dense float64 (N, 2) tensor on ``dev``"""
    if not torch.is_tensor(y):
        raise _lib.DcptHipError(f"{op} takes device tensors (got {type(y).__name__} for {name})")
    _require((y,), (torch.float64,), op + ": " + name + " must be float64 (got {})")
    if y.dim() != 2 or y.shape[1] != 2:
        raise ValueError(f"{op}: only two output dimensions exist; {name} must be ({N}, 2), got {tuple(y.shape)}")
    if y.shape[0] != N or y.device != dev or not y.is_contiguous():
        raise ValueError(f"{op}: {name} must be a contiguous ({N}, 2) tensor on {dev}, got {tuple(y.shape)} strides {y.stride()} on {y.device}")
    return y.detach()


def tsne_affinities(d2, perplexity, return_conditional=False):
    """The joint probabilities of exact t-SNE from a float64 (N, N) squared-distance device tensor with contiguous rows (what
    ``pairwise_sqdist`` returns): per row the binary search on beta for the given perplexity (at most 100 steps, tolerance 1e-5 on the
    entropy), then ``P = max((pcond + pcond^t) / sum, 2^-52)`` with a zero diagonal.  Returns ``(P, beta, steps)``: float64 (N, N),
    symmetric bit for bit; float64 (N,); int32 (N,) the index of the last search step of a row.  The diagonal of ``d2`` is never read, and
    the distances are not rounded to float32 as scikit-learn does.  ``return_conditional``: also return the conditional affinities of the
    search, float64 (N, N), as a fourth value.  Nothing is read back."""
    d2, ldd = _tsne_matrix("tsne_affinities", "d2", d2)
    N, dev, perplexity = d2.shape[0], d2.device, float(perplexity)
    if not (math.isfinite(perplexity) and 1.0 <= perplexity < N):
        raise ValueError(f"tsne_affinities: the perplexity must be finite and lie in [1, N = {N}), got {perplexity}")
    P = torch.empty((N, N), dtype=torch.float64, device=dev)
    beta = torch.empty(N, dtype=torch.float64, device=dev)
    steps = torch.empty(N, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nws = _check_ws("tsne_affinities", lib.dcpt_tsne_steps_ws_bytes(N), f"N={N}")
    ws = _workspace(dev, nws)
    pcond = torch.empty_like(P) if return_conditional else P   # (the joint pass may write over its input)
    _call(lib.dcpt_tsne_affinity_fwd, (d2, ldd, pcond, N, beta, steps), (N, perplexity), dev)
    _call(lib.dcpt_tsne_joint_fwd, (pcond, N, P, N, ws, nws), (N,), dev)
    return (P, beta, steps, pcond) if return_conditional else (P, beta, steps)


def tsne_steps(P, Y, update, gains, n_steps, exaggeration, momentum, lr, min_gain=0.01):
    """``n_steps`` descent iterations of exact t-SNE on ``Y``, ``update`` and ``gains`` (contiguous float64 (N, 2) device tensors), in
    place, with ``exaggeration * P`` for P, scikit-learn's gain rule (+0.2 / x0.8, floor ``min_gain``), ``momentum`` and step ``lr``.
    Returns ``stats``, a float64 device tensor of 2: the KL divergence at the Y before the last move and the norm of the last gain-scaled
    gradient.  Nothing is read back; with ``n_steps = 0`` nothing is launched and ``stats`` is NaN."""
    P, ldp = _tsne_matrix("tsne_steps", "P", P)
    N, dev = P.shape[0], P.device
    Y, update, gains = (_tsne_points("tsne_steps", n, t, N, dev) for n, t in (("Y", Y), ("update", update), ("gains", gains)))
    n_steps = int(n_steps)
    pars = tuple(float(v) for v in (exaggeration, momentum, lr, min_gain))
    if n_steps < 0 or not all(math.isfinite(v) for v in pars):
        raise ValueError(f"tsne_steps: n_steps must be at least 0 and exaggeration, momentum, lr, min_gain finite, got {n_steps} {pars}")
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    lib = _lib.load()
    nws = _check_ws("tsne_steps", lib.dcpt_tsne_steps_ws_bytes(N), f"N={N}")
    ws = _workspace(dev, nws)
    _call(lib.dcpt_tsne_steps_fwd, (P, ldp, Y, update, gains, stats, ws, nws), (N, 2, n_steps, *pars), dev)
    return stats


def tsne_kl(P, Y, exaggeration=1.0):
    """The KL divergence of exact t-SNE and its plain gradient at ``Y`` (contiguous float64 (N, 2) device tensor), which does not move:
    ``(kl, grad)``, a float64 device scalar and a float64 (N, 2) tensor, with ``exaggeration * P`` for P.  Nothing is read back."""
    P, ldp = _tsne_matrix("tsne_kl", "P", P)
    N, dev = P.shape[0], P.device
    Y = _tsne_points("tsne_kl", "Y", Y, N, dev)
    exaggeration = float(exaggeration)
    if not math.isfinite(exaggeration):
        raise ValueError(f"tsne_kl: the exaggeration must be finite, got {exaggeration}")
    grad = torch.empty((N, 2), dtype=torch.float64, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    lib = _lib.load()
    nws = _check_ws("tsne_kl", lib.dcpt_tsne_steps_ws_bytes(N), f"N={N}")
    ws = _workspace(dev, nws)
    _call(lib.dcpt_tsne_kl_fwd, (P, ldp, Y, grad, stats, ws, nws), (N, 2, exaggeration), dev)
    return stats[0], grad


# ------------------------------------------------------------------------------------------------
# MATLAB-bicubic resize and the pixel work of NIQE (include/dcpt_hip.h dcpt_imresize_fwd, dcpt_niqe_mscn_fwd, dcpt_niqe_block_stats_fwd):
# the reference's basicsr/utils/matlab_functions.py::imresize and the per-pixel part of basicsr/metrics/niqe.py in fp64.  Forward only.
IMRESIZE_X_F64, IMRESIZE_Y_F64, IMRESIZE_QUANT8 = 1, 2, 4   # include/dcpt_hip.h DCPT_IMRESIZE_*
_RESIZE_TABLES: Dict[tuple, tuple] = {}                    # (length, scale, antialiasing, device) -> (first int32 [out], weights fp64 [out][K])


def _resize_tables(n, scale, antialiasing, dev):
    key = (int(n), float(scale), bool(antialiasing), dev.type, dev.index)
    hit = _RESIZE_TABLES.get(key)
    if hit is None:
        from .matlab_resize import weights_indices

        first, weights = weights_indices(n, scale, antialiasing)   # (ValueError for an input shorter than the kernel reaches)
        hit = (torch.from_numpy(first).to(dev), torch.from_numpy(weights).to(dev))
        _RESIZE_TABLES[key] = hit
    return hit


def _imresize_planes(x, P, H, W, plane_stride, row_stride, scale, antialiasing, y, flags):
    """the resize of P planes read from ``x`` with the given strides into the dense ``y`` [P][Ho][Wo]; returns (Ho, Wo)"""
    lib = _lib.load()
    dev = x.device
    (fh, wh), (fw, ww) = _resize_tables(H, scale, antialiasing, dev), _resize_tables(W, scale, antialiasing, dev)
    Ho, Wo, Kh, Kw = fh.numel(), fw.numel(), wh.shape[1], ww.shape[1]
    if y is not None:
        if y.numel() != P * Ho * Wo or not y.is_contiguous():
            raise ValueError(f"imresize: the output must be a dense tensor of {P} x {Ho} x {Wo} elements, got {tuple(y.shape)}")
        nws = _check_ws("imresize", lib.dcpt_imresize_ws_bytes(P, H, W, Ho, Wo, Kh, Kw), f"P={P} H={H} W={W} -> {Ho} x {Wo}")
        ws = _workspace(dev, nws)
        _call(lib.dcpt_imresize_fwd, (x, y, fh, wh, fw, ww, ws, nws), (P, H, W, Ho, Wo, Kh, Kw, plane_stride, row_stride, flags), dev)
    return Ho, Wo


def imresize(x, scale, antialiasing=True, out_dtype=None):
    """``imresize`` of the reference (MATLAB bicubic, one scale for both axes) on a (B, C, H, W) device tensor, fp32 or fp64; returns
    (B, C, ceil(H scale), ceil(W scale)) of ``out_dtype`` (fp32 or fp64; default: the input's).  fp64 from the load to the one rounding at
    the store.  An input shorter than the kernel reaches raises ValueError."""
    if not torch.is_tensor(x):
        raise _lib.DcptHipError(f"imresize takes a device tensor (got {type(x).__name__}); host arrays go to basicsr.utils.imresize")
    _require((x,), (torch.float32, torch.float64), "imresize takes fp32 or fp64 planes (got {})")
    if x.dim() != 4:
        raise ValueError(f"imresize: expected a (B, C, H, W) tensor, got {tuple(x.shape)}")
    out_dtype = out_dtype or x.dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError(f"imresize: the output is fp32 or fp64 (got {out_dtype})")
    _inference_only("imresize", x, what="the MATLAB-bicubic resize")
    x = _contig(x.detach())
    B, Cc, H, W = x.shape
    Ho, Wo = _imresize_planes(x, B * Cc, H, W, H * W, W, scale, antialiasing, None, 0)
    y = torch.empty(B, Cc, Ho, Wo, dtype=out_dtype, device=x.device)
    flags = (IMRESIZE_X_F64 if x.dtype == torch.float64 else 0) | (IMRESIZE_Y_F64 if out_dtype == torch.float64 else 0)
    _imresize_planes(x, B * Cc, H, W, H * W, W, scale, antialiasing, y, flags)
    return y


def niqe_mscn(x, crop_border=0, scale=1, out=None):
    """the MSCN planes of one NIQE scale: ``scale=1`` takes the (P, H, W) fp32 image in [0, 1] (8-bit rounding, crop_border and the crop to
    whole 96 x 96 blocks by addressing), ``scale=2`` the (P, H, W) fp64 resize output; returns fp64 (P, Hc, Wc) (``out``: written in place)"""
    lib = _lib.load()
    _require((x,), (torch.float32,) if scale == 1 else (torch.float64,), "niqe_mscn: scale 1 reads fp32, scale 2 fp64 (got {})")
    if x.dim() != 3 or not x.is_contiguous():
        raise ValueError(f"niqe_mscn: expected dense (P, H, W) planes, got {tuple(x.shape)}")
    P, H, W = x.shape
    crop = int(crop_border)
    Hc, Wc = ((H - 2 * crop) // 96 * 96, (W - 2 * crop) // 96 * 96) if scale == 1 else (H, W)
    if out is None:
        out = torch.empty(P, max(Hc, 0), max(Wc, 0), dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or out.numel() != P * Hc * Wc or not out.is_contiguous():
        raise ValueError(f"niqe_mscn: out must be a dense fp64 tensor of {P} x {Hc} x {Wc} elements")
    _call(lib.dcpt_niqe_mscn_fwd, (x, out), (P, H, W, crop, int(scale)), x.device)
    return out


def niqe_block_stats(n, block, out=None):
    """fp64 MSCN planes (P, H, W), H and W multiples of ``block`` (96 or 48) -> the sums (P, nblk, 5, 6) fp64, blocks column-major"""
    lib = _lib.load()
    _require((n,), (torch.float64,), "niqe_block_stats reads fp64 MSCN planes (got {})")
    if n.dim() != 3 or not n.is_contiguous():
        raise ValueError(f"niqe_block_stats: expected dense (P, H, W) planes, got {tuple(n.shape)}")
    P, H, W = n.shape
    block = int(block)
    nblk = (H // block) * (W // block) if block > 0 else 0
    if out is None:
        out = torch.empty(P, nblk, 5, 6, dtype=torch.float64, device=n.device)
    elif out.dtype != torch.float64 or out.numel() != P * nblk * 30 or not out.is_contiguous():
        raise ValueError(f"niqe_block_stats: out must be a dense fp64 tensor of {P} x {nblk} x 5 x 6 elements")
    _call(lib.dcpt_niqe_block_stats_fwd, (n, out), (P, H, W, block), n.device)
    return out


def niqe_stats(img, crop_border=0, parts=False):
    """The pixel work of NIQE for a (B, C, H, W) fp32 device tensor in [0, 1]: returns the sums (B * C, nblk, 2, 5, 6) fp64 on the device
    -- scale 1 (96 x 96 blocks) and scale 2 (48 x 48 blocks of the x0.5 image) -- for basicsr.metrics.niqe.niqe_from_stats.  Five
    launches (MSCN, block sums, the two resize passes straight from the fp32 image, MSCN, block sums), nothing synchronises.  ``parts``:
    also {"mscn1", "img2", "mscn2"}, the intermediates (img2: the resize output in [0, 1])."""
    if not torch.is_tensor(img):
        raise _lib.DcptHipError(f"niqe_stats takes a device tensor (got {type(img).__name__}); host arrays go to basicsr.metrics.calculate_niqe")
    _require_gpu(img)
    if img.dim() != 4:
        raise ValueError(f"niqe_stats: expected a (B, C, H, W) tensor, got {tuple(img.shape)}")
    img = _contig(img.detach())
    B, Cc, H, W = img.shape
    P, crop = B * Cc, int(crop_border)
    if crop < 0 or (H - 2 * crop) // 96 < 1 or (W - 2 * crop) // 96 < 1:
        raise ValueError(f"niqe_stats: no whole 96 x 96 block in a {H} x {W} plane with crop_border {crop}")
    dev = img.device
    planes = img.view(P, H, W)
    n1 = niqe_mscn(planes, crop, 1)
    s1 = niqe_block_stats(n1, 96)
    Hc, Wc = n1.shape[1:]
    # the x0.5 image straight from the fp32 input: the cropped region by offset and strides, the 8-bit rounding at the load
    src = planes[:, crop:, crop:]
    x2 = torch.empty(P, Hc // 2, Wc // 2, dtype=torch.float64, device=dev)
    _imresize_planes(src, P, Hc, Wc, H * W, W, 0.5, True, x2, IMRESIZE_Y_F64 | IMRESIZE_QUANT8)
    n2 = niqe_mscn(x2, 0, 2, out=None if parts else n1.view(-1)[: x2.numel()].view(x2.shape))
    s2 = niqe_block_stats(n2, 48)
    stats = torch.stack((s1, s2), dim=2)
    return (stats, {"mscn1": n1, "img2": x2, "mscn2": n2}) if parts else stats
