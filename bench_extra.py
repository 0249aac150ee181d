#!/usr/bin/env python
"""Secondary workloads of BASELINE.json (configs[2..4]) on ONE MI355X -- evidence for DESIGN.md, not the driver's
contract (that is bench.py).  Prints one JSON line per workload.

    python bench_extra.py --workload dcpt|dcpt_swinir|restormer|promptir|infer2k|naf|swinir|rcan|val_metrics|val_metrics_ms|step_tail|tlsc|ssim_loss|ldl|jpeg|niqe|degrade|noise|blur|poisson|degrade_chain|knn|tsne [--dtype fp32|bf16|bf16_res32] [--steps K] [--warmup W]

``--dtype bf16`` (dcpt, naf, infer2k, restormer, promptir; rcan: the inference line only, next to fp32; swinir: the restoration form's inference, next to fp32): every feature map of the encoder in bf16 storage with fp32 accumulation (act_dtype="bf16";
dcpt: the classifier head too unless --head-dtype fp32); images, parameters and the optimizer stay fp32.  Its lines carry BOTH
rooflines: the bf16 MFMA peak (2.5 PF dense) and the HBM roof with the bf16 algorithmic bytes -- in bf16 the network is HBM-bound
(SURVEY 8d).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
NAF = dict(img_channel=3, width=64, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1])


def _barrier():
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize()


def timed(fn, steps, warmup):
    """W untimed steps, then K steps bracketed by barrier + synchronize on both sides; with several ranks the MAX over ranks"""
    import torch.distributed as dist

    for _ in range(warmup):
        fn()
    _barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    _barrier()
    dt = (time.perf_counter() - t0) / steps
    if dist.is_available() and dist.is_initialized():
        t = torch.tensor([dt], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


def run_restormer(dev, save="balanced", steps=5, warmup=2, B=64, S=128, rank=0, world=1, dtype="fp32", grad_clip=0.0, ema_decay=0.0,
                  fused_step_tail=False):
    """BASELINE.json configs[3]: Restormer defaults (reference restormer_arch.py:234-422), fwd + L1 + bwd (+ gradient all-reduce: the network
    in DistributedDataParallel as base_model.py:108-115 wraps it, when world > 1) + AdamW, fp32; dtype "bf16": act_dtype="bf16" (feature
    maps in bf16 storage, fp32 accumulation / parameters / optimizer), reported against the bf16 MFMA peak."""
    from basicsr.archs import build_network
    from dcpt_amd import functional as DF
    from dcpt_amd.keyed_init import fill_module_

    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    torch.cuda.reset_peak_memory_stats()
    DF.set_restormer_save(save)
    net = fill_module_(build_network(dict(type="Restormer", **({} if dtype == "fp32" else dict(act_dtype=dtype))))).to(dev)
    bare = net
    if world > 1:
        from torch.nn.parallel import DistributedDataParallel

        from dcpt_amd import ddp as dcpt_ddp

        net = dcpt_ddp.prepare(DistributedDataParallel(net, device_ids=[dev.index], bucket_cap_mb=64, gradient_as_bucket_view=True))
    from dcpt_amd.optim import FusedAdamW

    optm = FusedAdamW(bare.parameters(), lr=1e-4)
    lq = torch.rand((B, 3, S, S), generator=g, device=dev)
    gt = torch.rand((B, 3, S, S), generator=g, device=dev)

    # --grad-clip / --ema-decay: the step tail of SRModel.optimize_parameters (clip_grad_norm_, step, model_ema's foreach pair), or with
    # --fused-step-tail the one call of train.fused_step_tail
    params = list(bare.parameters())
    ema = [p.detach().clone() for p in params] if ema_decay > 0 else None
    ema_arg = (dict(zip(params, ema)), ema_decay) if ema is not None else None

    def step():
        optm.zero_grad(set_to_none=True)
        (net(lq) - gt).abs().mean().backward()
        if fused_step_tail:
            optm.step(max_grad_norm=grad_clip or None, ema=ema_arg)
            return
        if grad_clip:
            torch.nn.utils.clip_grad_norm_(params, grad_clip)
        optm.step()
        if ema is not None:
            torch._foreach_mul_(ema, ema_decay)
            torch._foreach_add_(ema, [p.detach() for p in params], alpha=1 - ema_decay)

    dt = timed(step, steps, warmup)
    flops = B * (S / 128.0) ** 2 * 232e9      # 77.45 GF fwd -> 232 GF fwd+bwd per 128^2 image
    peak = 2.5e15 if dtype == "bf16" else 157.3e12
    return dict(workload=f"Restormer (dim 48, [4,6,6,8], BiasFree LN) fwd+L1+bwd+AdamW, B={B}, {S}x{S}, {dtype}, saved tensors: {save} "
                         "(BASELINE.json configs[3])",
                ms_per_step=round(dt * 1e3, 2), megapixels_per_s=round(world * B * S * S / 1e6 / dt, 3), steps=steps, warmup=warmup,
                alg_tflops=round(flops / dt / 1e12, 2), mfma_frac=round(flops / dt / peak, 4),
                peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                **(dict(grad_clip=grad_clip, ema_decay=ema_decay, fused_step_tail=bool(fused_step_tail)) if (grad_clip or ema_decay) else {}))


def run_promptir(dev, save="balanced", steps=5, warmup=2, B=32, S=128, dtype="fp32"):
    """PromptIR defaults (dim 48, [4,6,6,8], 4 refinement blocks, WithBias LN, the 3 prompt blocks; the network behind
    options/all_in_one/test/test_PromptIR_5d.yml), fwd + L1 + bwd + FusedAdamW; dtype "bf16": act_dtype="bf16".  B = 32 at 128 x 128 by
    default: the fp32 step fits the device with room to spare."""
    from basicsr.archs import build_network
    from dcpt_amd import functional as DF
    from dcpt_amd.keyed_init import fill_module_
    from dcpt_amd.optim import FusedAdamW

    g = torch.Generator(device=dev).manual_seed(1234)
    torch.cuda.reset_peak_memory_stats()
    DF.set_restormer_save(save)
    net = fill_module_(build_network(dict(type="PromptIR", act_dtype=dtype))).to(dev)
    optm = FusedAdamW(net.parameters(), lr=1e-4)
    lq = torch.rand((B, 3, S, S), generator=g, device=dev)
    gt = torch.rand((B, 3, S, S), generator=g, device=dev)

    def step():
        optm.zero_grad(set_to_none=True)
        (net(lq) - gt).abs().mean().backward()
        optm.step()

    dt = timed(step, steps, warmup)
    return dict(workload=f"PromptIR (dim 48, [4,6,6,8], 4 refinement blocks, WithBias LN, 3 prompt blocks) fwd+L1+bwd+AdamW, B={B}, "
                         f"{S}x{S}, {dtype}, saved tensors: {save}",
                ms_per_step=round(dt * 1e3, 2), megapixels_per_s=round(B * S * S / 1e6 / dt, 3), steps=steps, warmup=warmup, batch=B,
                peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


SWINIR_5D = dict(embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)


def swinir_fwd_flops_per_pixel(embed_dim=180, depths=(6,) * 6, mlp_ratio=2.0, window_size=8, in_chans=3, **_):
    """per output pixel: every Swin block 2 (3C^2 + C^2 + 2 C hidden) for qkv / proj / fc1+fc2 and 4 ws^2 C for the window products
    (q k^T and p v), one 3 x 3 C -> C conv per RSTB and conv_after_body, the two edge convs"""
    C, hidden, n2 = embed_dim, int(embed_dim * mlp_ratio), window_size * window_size
    blocks = sum(depths) * (2 * (4 * C * C + 2 * C * hidden) + 4 * n2 * C)
    convs = (len(depths) + 1) * 2 * 9 * C * C + 2 * 2 * 9 * in_chans * C
    return blocks + convs


def swinir_sr_tail_macs_per_lr_pixel(upsampler, upscale, embed_dim=180, in_chans=3, num_feat=64):
    """forward MACs per LR pixel of everything after conv_after_body, each 3 x 3 conv at its own resolution (classical x4 at width 180:
    103 680 + 147 456 + 589 824 + 27 648 = 868 608; nearest+conv x4: 103 680 + 147 456 + 589 824 + 589 824 + 27 648 = 1 458 432)"""
    C, F, r = embed_dim, num_feat, upscale
    if upsampler == "":
        return 9 * C * in_chans
    if upsampler == "pixelshuffledirect":
        return 9 * C * r * r * in_chans
    macs, area = 9 * C * F, 1
    if upsampler == "pixelshuffle":
        for s in ([2] * (r.bit_length() - 1) if r & (r - 1) == 0 else [3]):
            macs += area * 9 * F * s * s * F
            area *= s * s
    else:
        for _ in range(r.bit_length() - 1):   # conv_up1 (, conv_up2) on the up-sampled grids
            area *= 4
            macs += area * 9 * F * F
        macs += area * 9 * F * F              # conv_hr
    return macs + area * 9 * F * in_chans


def run_swinir(dev, steps=5, warmup=2, B=8, S=256, train_batches=(12, 8, 4, 2, 1), upsampler="", upscale=1):
    """the 5D SwinIR (options/all_in_one/test/test_SwinIR_5d.yml) at S x S: inference at batch B, and one training step (fwd + L1 + bwd + AdamW)
    at the largest batch of ``train_batches`` that fits in device memory; rates against the fp32-MFMA roof.  With ``upsampler`` / ``upscale``:
    the same body with that super-resolution tail, S x S the LR size; FLOPs per LR pixel = the body's count with the restoration form's
    conv_last replaced by the tail's"""
    from basicsr.archs import build_network
    from dcpt_amd.keyed_init import fill_module_
    from dcpt_amd.optim import FusedAdamW

    g = torch.Generator(device=dev).manual_seed(1234)
    cfg = dict(SWINIR_5D, upsampler=upsampler, upscale=upscale)
    net = fill_module_(build_network(dict(type="SwinIR", **cfg))).to(dev)
    tail = 2 * swinir_sr_tail_macs_per_lr_pixel(upsampler, upscale, cfg["embed_dim"])
    fpp = swinir_fwd_flops_per_pixel(**SWINIR_5D) - 2 * swinir_sr_tail_macs_per_lr_pixel("", 1, cfg["embed_dim"]) + tail
    x = torch.rand((B, 3, S, S), generator=g, device=dev)

    def infer():
        with torch.no_grad():
            net(x)

    dt_inf = timed(infer, steps, warmup)
    del x
    torch.cuda.empty_cache()
    optm = FusedAdamW(net.parameters(), lr=1e-4)
    form = f" + {upsampler} x{upscale}, LR" if upsampler else ","
    res = dict(workload=f"SwinIR 5D (embed 180, depths [6]*6, heads [6]*6, ws 8, mlp 2){form} {S}x{S}, fp32",
               fwd_gflop_per_image=round(fpp * S * S / 1e9, 1), infer_batch=B, infer_ms_per_batch=round(dt_inf * 1e3, 2),
               infer_tflops=round(fpp * S * S * B / dt_inf / 1e12, 2), infer_mfma_frac=round(fpp * S * S * B / dt_inf / 157.3e12, 4),
               infer_roof_ms=round(fpp * S * S * B / 157.3e12 * 1e3, 1), steps=steps, warmup=warmup)
    if upsampler:
        res.update(tail_mmac_per_lr_pixel=round(tail / 2e6, 6), tail_flop_share=round(tail / fpp, 4))
    for tb in train_batches:
        try:
            lq = torch.rand((tb, 3, S, S), generator=g, device=dev)
            gt = torch.rand((tb, 3, upscale * S, upscale * S), generator=g, device=dev)

            def step():
                optm.zero_grad(set_to_none=True)
                (net(lq) - gt).abs().mean().backward()
                optm.step()

            torch.cuda.reset_peak_memory_stats()
            dt = timed(step, steps, warmup)
        except torch.cuda.OutOfMemoryError:
            lq = gt = None
            optm.zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
            continue
        flops = 3 * fpp * S * S * tb   # backward = 2 x forward (data and weight gradients)
        res.update(train_batch=tb, train_ms_per_step=round(dt * 1e3, 2), train_tflops=round(flops / dt / 1e12, 2),
                   train_mfma_frac=round(flops / dt / 157.3e12, 4), train_peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
        break
    return res


def run_swinir_bf16(dev, steps=5, warmup=2, B=8, S=256, res32=False):
    """the restoration-form inference of run_swinir on bf16 activation storage (SwinIR.set_act_dtype): fp32 and bf16 calls alternate in this
    process, the median per-call wall time of each (one synchronize per call), the peak memory of one call above the resident state (weights,
    padded operand caches, workspaces) and the kernel launches of one bf16 call from the library's launch trace.  The protocol of
    ``--workload rcan --dtype bf16``.  ``res32`` (--dtype bf16_res32): bf16_res32 calls (the fp32 residual stream) alternate with the two as
    a third mode, and the line carries its median, minimum and peak memory as well."""
    import ctypes

    from basicsr.archs import build_network
    from dcpt_amd import _lib
    from dcpt_amd.keyed_init import fill_module_

    g = torch.Generator(device=dev).manual_seed(1234)
    net = fill_module_(build_network(dict(type="SwinIR", **SWINIR_5D))).to(dev).eval()
    fpp = swinir_fwd_flops_per_pixel(**SWINIR_5D)
    x = torch.rand((B, 3, S, S), generator=g, device=dev)

    def infer():
        with torch.no_grad():
            net(x)

    modes = ("fp32", "bf16_res32", "bf16") if res32 else ("fp32", "bf16")
    times, peaks = {act: [] for act in modes}, {}
    for act in modes:   # warm the paths (workspaces, operand caches), then the peak of one call above what stays resident
        net.set_act_dtype(act)
        for _ in range(max(warmup, 1)):
            infer()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        infer()
        torch.cuda.synchronize()
        peaks[act] = torch.cuda.max_memory_allocated() - base
    lib = _lib.load()
    lib.dcpt_trace_enable(1)   # (net is in bf16 mode here)
    infer()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(int(lib.dcpt_trace_read(None, 0)) + 16)
    lib.dcpt_trace_read(buf, len(buf))
    lib.dcpt_trace_enable(0)
    tags = {ln.rpartition(" ")[0]: int(ln.rpartition(" ")[2]) for ln in buf.value.decode().splitlines() if ln.strip()}
    # one tag per launch: the padded LayerNorm, the window kernel, every GEMM by its tile class, the two edge convs; + the two img_affine
    launches = 2 + sum(v for k, v in tags.items() if k in ("swin_bf16.ln_pad_fwd", "swin_bf16.wattn_fwd", "edge.s2b_bf16", "edge.b2s_bf16")
                       or (k.startswith("nt_bf16.") and ".epi_" not in k))
    for _ in range(steps):
        for act in modes:
            net.set_act_dtype(act)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            infer()
            torch.cuda.synchronize()
            times[act].append(time.perf_counter() - t0)
    net.set_act_dtype("fp32")
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    f = fpp * S * S * B
    extra = {}
    if res32:
        extra = dict(modes=list(modes), infer_ms_per_batch_bf16_res32=round(med["bf16_res32"] * 1e3, 2),
                     infer_ms_per_batch_bf16_res32_min=round(min(times["bf16_res32"]) * 1e3, 2),
                     bf16_res32_speedup=round(med["fp32"] / med["bf16_res32"], 3), peak_act_mem_mb_bf16_res32=round(peaks["bf16_res32"] / 2 ** 20, 1))
    return dict(workload=f"SwinIR 5D (embed 180 -> rows of {net.padded_dim()}, depths [6]*6, heads [6]*6, ws 8, mlp 2) inference, {B} x {S}x{S}, "
                         "fp32 and bf16 storage alternating",
                fwd_gflop_per_image=round(fpp * S * S / 1e9, 1), infer_batch=B, infer_ms_per_batch=round(med["fp32"] * 1e3, 2),
                infer_ms_per_batch_bf16=round(med["bf16"] * 1e3, 2), infer_ms_per_batch_min=round(min(times["fp32"]) * 1e3, 2),
                infer_ms_per_batch_bf16_min=round(min(times["bf16"]) * 1e3, 2), bf16_speedup=round(med["fp32"] / med["bf16"], 3),
                infer_tflops=round(f / med["fp32"] / 1e12, 2), infer_tflops_bf16=round(f / med["bf16"] / 1e12, 2),
                peak_act_mem_mb=round(peaks["fp32"] / 2 ** 20, 1), peak_act_mem_mb_bf16=round(peaks["bf16"] / 2 ** 20, 1),
                launches_per_call_bf16=launches, window_kernel_launches=tags.get("swin_bf16.wattn_fwd", 0),
                timing="median of per-call wall times, one synchronize per call", steps=steps, warmup=warmup, **extra)


def rcan_fwd_flops_per_lr_pixel(num_in_ch=3, num_out_ch=3, num_feat=64, num_group=10, num_block=16, upscale=4, **_):
    """per LR pixel: 2 per MAC of every 3 x 3 conv at its own resolution -- the two convs of every RCAB, the group convs and
    conv_after_body (C -> C), conv_first, each Upsample stage (C -> r^2 C at its input resolution) and conv_last at the HR resolution;
    the channel attention's pooling and FCs are per image, not per pixel, and left out"""
    C = num_feat
    body = (num_group * (2 * num_block + 1) + 1) * 2 * 9 * C * C
    stages = [2] * (upscale.bit_length() - 1) if upscale & (upscale - 1) == 0 else [3]
    up, area = 0, 1
    for r in stages:
        up += area * 2 * 9 * C * r * r * C
        area *= r * r
    return body + 2 * 9 * num_in_ch * C + up + area * 2 * 9 * C * num_out_ch


def run_rcan(dev, steps=5, warmup=2, B=16, S=48, S_inf=256, dtype="fp32"):
    """the default x4 RCAN (64 features, 10 x 16 RCABs): one training step (fwd + L1 + bwd + AdamW) at B x S^2 LR patches, and inference of
    one S_inf^2 LR image; rates against the fp32-MFMA roof from the FLOPs counted above.  ``dtype="bf16"``: the inference line also holds the
    same network on bf16 activation storage (set_act_dtype), fp32 and bf16 images alternating in this process, with the peak memory of each
    above the resident state (weights, weight packs, workspaces); training stays fp32 (there is no bf16 backward).  ``dtype="bf16_res32"``:
    the same with bf16_res32 images (the fp32 residual stream) alternating as a third mode"""
    from basicsr.archs import build_network
    from dcpt_amd.keyed_init import fill_module_
    from dcpt_amd.optim import FusedAdamW

    cfg = dict(num_in_ch=3, num_out_ch=3)
    g = torch.Generator(device=dev).manual_seed(1234)
    net = fill_module_(build_network(dict(type="RCAN", **cfg))).to(dev)
    fpp = rcan_fwd_flops_per_lr_pixel(**cfg)
    optm = FusedAdamW(net.parameters(), lr=1e-4)
    lq = torch.rand((B, 3, S, S), generator=g, device=dev)
    gt = torch.rand((B, 3, 4 * S, 4 * S), generator=g, device=dev)

    def step():
        optm.zero_grad(set_to_none=True)
        (net(lq) - gt).abs().mean().backward()
        optm.step()

    dt = timed(step, steps, warmup)
    flops = 3 * fpp * S * S * B   # backward = 2 x forward (data and weight gradients)
    train = dict(workload=f"RCAN x4 (64 feat, 10 groups x 16 RCABs) fwd+L1+bwd+AdamW, B={B}, {S}x{S} LR -> {4 * S}x{4 * S}, fp32",
                 fwd_mflop_per_lr_pixel=round(fpp / 1e6, 3), ms_per_step=round(dt * 1e3, 2), alg_tflops=round(flops / dt / 1e12, 2),
                 mfma_frac=round(flops / dt / 157.3e12, 4), roof_ms=round(flops / 157.3e12 * 1e3, 2), steps=steps, warmup=warmup)
    optm.zero_grad(set_to_none=True)
    del lq, gt
    torch.cuda.empty_cache()
    x = torch.rand((1, 3, S_inf, S_inf), generator=g, device=dev)

    def infer():
        with torch.no_grad():
            net(x)

    dt_inf = timed(infer, steps, warmup)
    f_inf = fpp * S_inf * S_inf
    infer_line = dict(workload=f"RCAN x4 inference, 1 x {S_inf}x{S_inf} LR -> {4 * S_inf}x{4 * S_inf}, fp32",
                      fwd_mflop_per_lr_pixel=round(fpp / 1e6, 3), ms_per_image=round(dt_inf * 1e3, 2), alg_tflops=round(f_inf / dt_inf / 1e12, 2),
                      mfma_frac=round(f_inf / dt_inf / 157.3e12, 4), roof_ms=round(f_inf / 157.3e12 * 1e3, 2), steps=steps, warmup=warmup)
    if dtype in ("bf16", "bf16_res32"):
        modes = ("fp32", "bf16_res32", "bf16") if dtype == "bf16_res32" else ("fp32", "bf16")
        times, peaks = {act: [] for act in modes}, {}
        for act in modes:   # warm the paths (workspaces, weight packs), then the peak of one image above what stays resident
            net.set_act_dtype(act)
            for _ in range(max(warmup, 1)):
                infer()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            infer()
            torch.cuda.synchronize()
            peaks[act] = torch.cuda.max_memory_allocated() - base
        for _ in range(steps):
            for act in modes:
                net.set_act_dtype(act)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                infer()
                torch.cuda.synchronize()
                times[act].append(time.perf_counter() - t0)
        net.set_act_dtype("fp32")
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        infer_line.update(workload=f"RCAN x4 inference, 1 x {S_inf}x{S_inf} LR -> {4 * S_inf}x{4 * S_inf}, fp32 and bf16 storage alternating",
                          ms_per_image=round(med["fp32"] * 1e3, 2), ms_per_image_bf16=round(med["bf16"] * 1e3, 2),
                          ms_per_image_min=round(min(times["fp32"]) * 1e3, 2), ms_per_image_bf16_min=round(min(times["bf16"]) * 1e3, 2),
                          bf16_speedup=round(med["fp32"] / med["bf16"], 3), alg_tflops=round(f_inf / med["fp32"] / 1e12, 2),
                          alg_tflops_bf16=round(f_inf / med["bf16"] / 1e12, 2), mfma_frac=round(f_inf / med["fp32"] / 157.3e12, 4),
                          peak_act_mem_mb=round(peaks["fp32"] / 2 ** 20, 1), peak_act_mem_mb_bf16=round(peaks["bf16"] / 2 ** 20, 1),
                          timing="median of per-image wall times, one synchronize per image")
        if dtype == "bf16_res32":
            infer_line.update(modes=list(modes), ms_per_image_bf16_res32=round(med["bf16_res32"] * 1e3, 2),
                              ms_per_image_bf16_res32_min=round(min(times["bf16_res32"]) * 1e3, 2),
                              bf16_res32_speedup=round(med["fp32"] / med["bf16_res32"], 3),
                              peak_act_mem_mb_bf16_res32=round(peaks["bf16_res32"] / 2 ** 20, 1))
    return [train, infer_line]


def run_infer2k(dev, dtype="fp32", steps=5, warmup=2, S=2048, streams=2):
    """BASELINE.json configs[4]: one S x S image through SRModel.test_tile (reference sr_model.py:273-361), 512-pixel tiles with 16 pixels
    of context, NAFNet-64 inference."""
    from basicsr.models import build_model
    from dcpt_amd.keyed_init import fill_module_

    g = torch.Generator(device=dev).manual_seed(1234)
    torch.cuda.reset_peak_memory_stats()
    peak = 2.5e15 if dtype.startswith("bf16") else 157.3e12
    opt = dict(name="b", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
               network_g=dict(type="NAFNetBaseline", window_size=16, **dict(NAF, act_dtype=dtype)), path=dict(),
               tile=dict(infer_size=512, tile_pad=16, streams=streams), val=dict(save_img=False))
    m = build_model(opt)
    fill_module_(m.net_g)
    img = torch.rand((1, 3, S, S), generator=g, device=dev)

    def run():
        m.feed_data({"lq": img})
        m.pre_test()
        m.test_tile()
        m.post_test()

    dt = timed(run, steps, warmup)
    flops = (S / 256.0) ** 2 * 126.11e9 * (544 / 512.0) ** 2
    return dict(workload=f"NAFNet-64 tiled inference, {S}x{S}, test_tile infer_size 512 / tile_pad 16, feature maps {dtype} "
                         f"(BASELINE.json configs[4]), tile batches on {streams} stream(s)",
                ms_per_image=round(dt * 1e3, 2), megapixels_per_s=round(S * S / 1e6 / dt, 3), steps=steps, warmup=warmup,
                alg_tflops=round(flops / dt / 1e12, 2), mfma_peak_tflops=peak / 1e12, mfma_frac=round(flops / dt / peak, 4),
                peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def run_tlsc(dev, steps=5, warmup=2, H=1080, W=2048, tile=0, streams=2, dtypes=("fp32", "bf16", "bf16_tail32", "bf16_edge32")):
    """The reference's large-image variant, ``NAFNet`` (TLSC: every SCA mean a local box mean of 1.5 x train_size, scaled per level; reference
    nafnet_arch.py:277-288), NAFNet-64 with train_size 256 on one 3 x H x W image, in all four feature-map storage modes: whole image
    (pre_test pads to a multiple of 16) or, with ``tile`` > 0, through SRModel.test_tile with tile_pad 16.  ms per image per mode, the fp32
    number of the same run as the baseline."""
    from basicsr.models import build_model
    from dcpt_amd import functional as DF
    from dcpt_amd.keyed_init import fill_module_

    g = torch.Generator(device=dev).manual_seed(1234)
    img = torch.rand((1, 3, H, W), generator=g, device=dev)
    ms, mem = {}, {}
    for dt in dtypes:
        torch.cuda.reset_peak_memory_stats()
        opt = dict(name="b", model_type="SRModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=False,
                   network_g=dict(type="NAFNet", train_size=(1, 3, 256, 256), window_size=16, **dict(NAF, act_dtype=dt)), path=dict(),
                   val=dict(save_img=False))
        if tile:
            opt["tile"] = dict(infer_size=tile, tile_pad=16, streams=streams)
        m = build_model(opt)
        fill_module_(m.net_g)

        def run():
            m.feed_data({"lq": img})
            m.pre_test()
            m.test_tile() if tile else m.test()
            m.post_test()

        ms[dt] = round(timed(run, steps, warmup) * 1e3, 2)
        mem[dt] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        del m
        DF.release_workspaces()
        torch.cuda.empty_cache()
    how = f"test_tile infer_size {tile} / tile_pad 16 on {streams} stream(s)" if tile else "whole image"
    base = ms.get("fp32")
    return dict(workload=f"NAFNet-64 TLSC inference (NAFNet, train_size 256), 3x{H}x{W}, {how}", ms_per_image=ms,
                speedup_vs_fp32={k: round(base / v, 2) for k, v in ms.items()} if base else None, peak_mem_gb_per_mode=mem, steps=steps,
                warmup=warmup)


def run_val_metrics(dev, steps=5, warmup=2, H=1080, W=2048):
    """PSNR + SSIM of one 3 x H x W pair as validation scores it (crop_border 0, RGB, image_range 255): the host functions of
    basicsr.metrics on the arrays SRModel.get_current_visuals hands them (one repetition, its three device-to-host copies included)
    against calculate_psnr_device / calculate_ssim_device's kernel on the tensors where they are (sums fetched in one transfer)."""
    from basicsr.metrics import MetricSums, calculate_psnr, calculate_ssim

    g = torch.Generator(device=dev).manual_seed(1234)
    gt = torch.rand((1, 3, H, W), generator=g, device=dev)
    out = (gt + 0.05 * torch.randn((1, 3, H, W), generator=g, device=dev)).clamp(0, 1)
    lq = torch.rand((1, 3, H, W), generator=g, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, res_h, gt_h = lq.cpu(), out.cpu().clamp(0, 1).numpy(), gt.cpu().clamp(0, 1).numpy()
    t_copy = time.perf_counter() - t0
    psnr_h = calculate_psnr(res_h, gt_h, 0)
    t_psnr = time.perf_counter() - t0 - t_copy
    ssim_h = calculate_ssim(res_h, gt_h, 0)
    t_host = time.perf_counter() - t0
    vals = {}

    def device():
        acc = MetricSums(crop_border=0)
        acc.add(out.clamp(0, 1), gt.clamp(0, 1))
        vals.update(acc.result())

    dt = timed(device, steps, warmup)
    return dict(workload=f"validation metrics of one 3 x {H} x {W} pair: PSNR + SSIM, crop_border 0, RGB, image_range 255",
                host_ms=round(t_host * 1e3, 2), host_copy_ms=round(t_copy * 1e3, 2), host_psnr_ms=round(t_psnr * 1e3, 2),
                host_ssim_ms=round((t_host - t_copy - t_psnr) * 1e3, 2), host_repetitions=1,
                device_ms=round(dt * 1e3, 3), steps=steps, warmup=warmup, psnr_host=psnr_h, psnr_device=vals["psnr"][0], ssim_host=ssim_h,
                ssim_device=vals["ssim"][0], note="device_ms: clamp of both images + two launches + one 32-byte transfer, host clock around "
                                                  "a synchronised region")


def run_val_metrics_ms(dev, steps=5, warmup=2, H=1080, W=2048):
    """MS-SSIM, MATLAB SSIM and NRMSE of one 3 x H x W pair (crop_border 0, RGB, image_range 255), one JSON line each: the host function of
    basicsr.metrics on the arrays SRModel.get_current_visuals hands it (one repetition, the copies timed apart) against the device function
    (kernels of dcpt_amd/csrc/metrics_ms.hip, sums fetched in one transfer) and against the same arithmetic as float64 torch expressions
    on the device (F.conv2d with the outer-product window, F.pad(mode="replicate"); value fetched with one .item())."""
    import torch.nn.functional as F

    from basicsr.metrics import (MSSSIM_WEIGHTS, calculate_msssim, calculate_msssim_device, calculate_nrmse, calculate_nrmse_device,
                                 calculate_ssim_matlab, calculate_ssim_matlab_device)

    g = torch.Generator(device=dev).manual_seed(1234)
    gt = torch.rand((1, 3, H, W), generator=g, device=dev)
    out = (gt + 0.05 * torch.randn((1, 3, H, W), generator=g, device=dev)).clamp(0, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res_h, gt_h = out.cpu().numpy(), gt.cpu().numpy()
    t_copy = time.perf_counter() - t0
    k1 = torch.exp(-((torch.arange(11, dtype=torch.float64, device=dev) - 5.0) ** 2) / (2 * 1.5 ** 2))
    k1 = k1 / k1.sum()
    win = torch.outer(k1, k1).view(1, 1, 11, 11)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    quant = lambda t: (t * 255.0).round().double()  # noqa: E731

    def moments(x, y, w):
        cv = lambda t: F.conv2d(t, w, groups=w.shape[0])  # noqa: E731
        mu1, mu2 = cv(x), cv(y)
        return mu1 * mu1, mu2 * mu2, mu1 * mu2, cv(x * x) - mu1 * mu1, cv(y * y) - mu2 * mu2, cv(x * y) - mu1 * mu2

    def blur(t):
        p = F.pad(t, (0, 1, 0, 1), mode="replicate")
        return 0.25 * ((p[..., :-1, :-1] + p[..., :-1, 1:]) + (p[..., 1:, :-1] + p[..., 1:, 1:]))

    def torch_msssim():
        x, y, v = quant(out), quant(gt), 1.0
        for k, wk in enumerate(MSSSIM_WEIGHTS):
            m1, m2, m12, s1, s2, s12 = moments(x[:, k % 3:k % 3 + 1], y[:, k % 3:k % 3 + 1], win)
            cs = (2 * s12 + c2) / (s1 + s2 + c2)
            last = k == len(MSSSIM_WEIGHTS) - 1
            v = v * ((((2 * m12 + c1) / (m1 + m2 + c1)) * cs).mean() if last else cs.mean()) ** wk
            if not last:
                x, y = blur(x), blur(y)
        return v.item()

    def torch_matlab():
        pad = lambda t: F.pad(t, (5, 5, 5, 5), mode="replicate")  # noqa: E731
        m1, m2, m12, s1, s2, s12 = moments(pad(quant(out)), pad(quant(gt)), win.expand(3, 1, 11, 11))
        per = (((2 * m12 + c1) * (2 * s12 + c2)) / ((m1 + m2 + c1) * (s1 + s2 + c2))).mean(dim=(0, 2, 3))
        return ((per.sum() + per[-1]) / 4).item()

    def torch_nrmse():
        x, y = quant(out), quant(gt)
        return (((x - y) ** 2).mean().sqrt() / (x.max() - x.min())).item()

    lines = []
    for name, host_fn, dev_fn, torch_fn in (("MS-SSIM (5 levels)", calculate_msssim, calculate_msssim_device, torch_msssim),
                                            ("MATLAB SSIM", calculate_ssim_matlab, calculate_ssim_matlab_device, torch_matlab),
                                            ("NRMSE", calculate_nrmse, calculate_nrmse_device, torch_nrmse)):
        t0 = time.perf_counter()
        v_host = host_fn(res_h, gt_h, 0)
        t_host = time.perf_counter() - t0
        vals = {}
        dt_dev = timed(lambda: vals.update(device=dev_fn(out, gt, 0)), steps, warmup)
        dt_torch = timed(lambda: vals.update(torch=torch_fn()), steps, warmup)
        lines.append(dict(workload=f"validation metric of one 3 x {H} x {W} pair: {name}, crop_border 0, RGB, image_range 255",
                          host_ms=round(t_host * 1e3, 2), host_copy_ms=round(t_copy * 1e3, 2), host_repetitions=1,
                          device_ms=round(dt_dev * 1e3, 3), torch_fp64_ms=round(dt_torch * 1e3, 3), steps=steps, warmup=warmup,
                          value_host=v_host, value_device=vals["device"], value_torch_fp64=vals["torch"],
                          note="host_ms excludes host_copy_ms (the two device-to-host copies the host route needs, shared by the three "
                               "metrics); device_ms / torch_fp64_ms: host clock around a synchronised region, the result fetched each step"))
    return lines


def run_step_tail(dev, steps=50, warmup=5, rounds=7, max_norm=1.0, decay=0.999):
    """The tail of a fine-tuning step (reference sr_model.py:166-174) on the parameter list of NAFNet-64 [1,1,1,28] -- shapes only, no
    forward, random gradients: clip_grad_norm_ + FusedAdamW.step() + the _foreach_mul_ / _foreach_add_ pair of model_ema (the torch route)
    against the one call FusedAdamW.step(max_grad_norm=, ema=).  Each on its own copy of the list, alternating, ``rounds`` windows of
    ``steps`` steps each, the median window of each; launch counts of one step from the library's launch trace (it sees the library's
    kernels only: the foreach kernels of the torch route are not in it)."""
    import ctypes
    import statistics

    from basicsr.archs import build_network
    from dcpt_amd import _lib
    from dcpt_amd.optim import FusedAdamW

    shapes = [tuple(p.shape) for p in build_network(dict(type="NAFNetBaseline", **NAF)).parameters()]
    g = torch.Generator(device=dev).manual_seed(1234)

    def make():
        ps = [torch.nn.Parameter(torch.randn(s, generator=g, device=dev) * 0.05) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-3
        return ps, [p.detach().clone() for p in ps], FusedAdamW(ps, lr=1e-4, betas=(0.9, 0.9), weight_decay=0.0)

    (pa, ea, oa), (pb, eb, ob) = make(), make()
    ema_b = (dict(zip(pb, eb)), decay)

    def torch_route_plain():
        torch.nn.utils.clip_grad_norm_(pa, max_norm)
        oa.step()
        torch._foreach_mul_(ea, decay)
        torch._foreach_add_(ea, [p.detach() for p in pa], alpha=1 - decay)

    def fused():
        ob.step(max_grad_norm=max_norm, ema=ema_b)

    def trace(fn):
        lib = _lib.load()
        lib.dcpt_trace_enable(1)
        fn()
        need = lib.dcpt_trace_read(None, 0)
        buf = ctypes.create_string_buffer(int(need) + 16)
        lib.dcpt_trace_read(buf, len(buf))
        lib.dcpt_trace_enable(0)
        return {ln.rpartition(" ")[0]: int(ln.rpartition(" ")[2]) for ln in buf.value.decode().splitlines() if ln.strip()}

    for fn in (torch_route_plain, fused):
        for _ in range(warmup):
            fn()
    launches_torch, launches_fused = trace(torch_route_plain), trace(fused)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(torch_route_plain, steps, 1))
        tb.append(timed(fused, steps, 1))
    numel = sum(p.numel() for p in pa)
    mt, mf = statistics.median(ta), statistics.median(tb)
    return dict(workload=f"step tail on the NAFNet-64 [1,1,1,28] parameter list ({len(shapes)} tensors, {numel / 1e6:.1f} M parameters): clip + AdamW + EMA",
                torch_route_ms=round(mt * 1e3, 4), fused_ms=round(mf * 1e3, 4), ratio=round(mt / mf, 3),
                torch_route_ms_windows=[round(t * 1e3, 4) for t in ta], fused_ms_windows=[round(t * 1e3, 4) for t in tb],
                steps_per_window=steps, rounds=rounds, library_launches_torch_route=launches_torch, library_launches_fused=launches_fused,
                alg_gbytes_torch_route=round(15 * 4 * numel / 1e9, 2), alg_gbytes_fused=round(10 * 4 * numel / 1e9, 2),
                fused_hbm_frac=round(10 * 4 * numel / mf / 8e12, 4),
                note="torch route = clip_grad_norm_ + FusedAdamW.step() + _foreach_mul_/_foreach_add_; host clock around synchronised windows, "
                     "the two routes alternating in one process; max_norm below the gradient norm: both routes multiply every gradient")


def run_ssim_loss(dev, steps=20, warmup=3, B=32, S=256):
    """SSIMMSELoss forward + backward at B x 3 x S x S (the loss alone: ``pred`` is a leaf): the kernel route (basicsr.losses.SSIMMSELoss,
    dcpt_amd/csrc/ssim_loss.hip) against a torch route on the device, the reference's arithmetic as it stands there -- five grouped 11 x 11
    fp64 ``F.conv2d`` passes and autograd's transposes.  The two alternate call by call in one process; each call is bracketed by device
    events; median and minimum of the per-call times after the warm-up.  If the torch route cannot run on the device its error text is
    recorded instead."""
    import statistics

    import numpy as np
    import torch.nn.functional as F

    from basicsr.losses import SSIMMSELoss

    g = torch.Generator(device=dev).manual_seed(1234)
    target = torch.rand((B, 3, S, S), generator=g, device=dev)
    pred = (target + 0.05 * torch.randn((B, 3, S, S), generator=g, device=dev)).clamp(0, 1).requires_grad_(True)
    crit = SSIMMSELoss()
    x = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(x ** 2) / (2 * 1.5 ** 2))
    k /= k.sum()
    win = torch.from_numpy(np.outer(k, k)).to(dev).view(1, 1, 11, 11).expand(3, 1, 11, 11).contiguous()
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def torch_loss():
        a, b = pred.double(), target.double()
        cv = lambda t: F.conv2d(t, win, groups=3)   # noqa: E731
        mu1, mu2 = cv(a), cv(b)
        mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s1, s2, s12 = cv(a * a) - mu1_sq, cv(b * b) - mu2_sq, cv(a * b) - mu12
        ssim = (((2 * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * ((2 * s12 + c2) / (s1 + s2 + c2))).mean([1, 2, 3])
        return 0.1 * (1 - ssim.mean()) + F.mse_loss(pred, target)

    vals = {}

    def call(name, fn):
        pred.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = fn()
        loss.backward()
        e1.record()
        e1.synchronize()
        vals[name] = float(loss.detach())
        return e0.elapsed_time(e1)

    routes = {"kernel": lambda: crit(pred, target), "torch": torch_loss}
    torch_error = None
    try:
        call("torch", torch_loss)
    except Exception as e:  # noqa: BLE001  (recorded, not hidden: the line then holds the kernel route alone)
        torch_error = f"{type(e).__name__}: {e}"[:400]
        routes.pop("torch")
    times = {n: [] for n in routes}
    for i in range(warmup + steps):
        for n, fn in routes.items():
            t = call(n, fn)
            if i >= warmup:
                times[n].append(t)
    res = dict(workload=f"SSIMMSELoss forward + backward, {B} x 3 x {S} x {S}, fp64 SSIM term, loss alone (pred is a leaf)",
               kernel_ms_median=round(statistics.median(times["kernel"]), 4), kernel_ms_min=round(min(times["kernel"]), 4),
               kernel_share_of_117ms_fp32_step=round(statistics.median(times["kernel"]) / 117.0, 4), loss_kernel=vals["kernel"],
               calls=steps, warmup=warmup, plane_cap_mib=64,
               note="device events around each forward + backward call, the two routes alternating in one process; "
                    "117 ms: the fp32 NAFNet-64 step of bench.py the loss would join")
    if torch_error is None:
        res.update(torch_ms_median=round(statistics.median(times["torch"]), 4), torch_ms_min=round(min(times["torch"]), 4),
                   ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 2), loss_torch=vals["torch"])
    else:
        res["torch_route_error"] = torch_error
    return res


def run_ldl(dev, steps=20, warmup=3, B=32, S=256):
    """The LDL term alone at B x 3 x S x S, ``out`` a leaf: ``w = get_refined_artifact_map(gt, out, std=True); (w * |out - gt|).mean()
    .backward()``.  The kernel route (basicsr.losses.loss_util, dcpt_amd/csrc/ldl.hip) against a torch route on the device: the reference's
    expression as it runs there, in fp32 -- F.pad(reflect), unfold(7).unfold(7), torch.std, the standardisation and the tanh under autograd.
    The two alternate call by call in one process; each call is bracketed by device events; median and minimum of the per-call times after
    the warm-up, and each route's peak memory above what is resident between calls.  If the torch route cannot run at B its error text is
    recorded and it is timed at the largest of B / 2, B / 4, .. at which it runs."""
    import statistics

    import torch.nn.functional as F

    from basicsr.losses.loss_util import get_refined_artifact_map

    g = torch.Generator(device=dev).manual_seed(1234)
    gt = torch.rand((B, 3, S, S), generator=g, device=dev)
    out = (gt + 0.05 * torch.randn((B, 3, S, S), generator=g, device=dev)).requires_grad_(True)

    def kernel_loss(o, t):
        return (get_refined_artifact_map(t, o, std=True) * (o - t).abs()).mean()

    def torch_loss(o, t):
        r = (t - o).abs()
        win = F.pad(r, [3, 3, 3, 3], mode="reflect").unfold(2, 7, 1).unfold(3, 7, 1)
        u = torch.std(win, dim=(-1, -2), unbiased=True)
        u = (u - u.mean()) / u.std()
        return ((u.tanh() + 1) / 2 * (o - t).abs()).mean()

    vals, peaks = {}, {}

    def call(name, fn, nb):
        o, t = (out, gt) if nb == B else (out_small, gt[:nb])
        o.grad = None
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = fn(o, t)
        loss.backward()
        e1.record()
        e1.synchronize()
        vals[name] = float(loss.detach())
        peaks[name] = max(peaks.get(name, 0), torch.cuda.max_memory_allocated(dev) - base)
        return e0.elapsed_time(e1)

    torch_errors, tb, out_small = [], B, None
    while tb >= 1:
        out_small = out if tb == B else out.detach()[:tb].clone().requires_grad_(True)
        try:
            call("torch", torch_loss, tb)
            break
        except Exception as e:  # noqa: BLE001  (recorded, not hidden)
            torch_errors.append(f"batch {tb}: {type(e).__name__}: {e}"[:300])
            out_small = None
            torch.cuda.empty_cache()
            tb //= 2
    routes = {"kernel": (kernel_loss, B)}
    if tb >= 1:
        routes["torch"] = (torch_loss, tb)
    peaks.clear()
    times = {n: [] for n in routes}
    for i in range(warmup + steps):
        for n, (fn, nb) in routes.items():
            t = call(n, fn, nb)
            if i >= warmup:
                times[n].append(t)
    res = dict(workload=f"LDL term forward + backward, {B} x 3 x {S} x {S}: w = get_refined_artifact_map(gt, out, std=True); "
                        f"(w * |out - gt|).mean().backward(), out a leaf",
               kernel_ms_median=round(statistics.median(times["kernel"]), 4), kernel_ms_min=round(min(times["kernel"]), 4),
               kernel_peak_mb=round(peaks["kernel"] / 1e6, 1), loss_kernel=vals["kernel"], calls=steps, warmup=warmup,
               note="device events around each forward + backward call, the two routes alternating in one process; peak memory of a call "
                    "above what is allocated between calls; the torch route is the reference's fp32 expression under autograd")
    if "torch" in routes:
        res.update(torch_batch=tb, torch_ms_median=round(statistics.median(times["torch"]), 4), torch_ms_min=round(min(times["torch"]), 4),
                   torch_peak_mb=round(peaks["torch"] / 1e6, 1), loss_torch=vals["torch"],
                   ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 2))
    if torch_errors:
        res["torch_route_errors"] = torch_errors
    return res


def run_jpeg(dev, steps=20, warmup=3, B=32, S=256):
    """The JPEG round trip of a B x 3 x S x S batch with one quality per image (10 / 20 / 30 / 40 in turn), ``uint8_io`` off: the kernel
    route (dcpt_amd.functional.diffjpeg, dcpt_amd/csrc/jpeg.hip) against a torch route on the device, the reference DiffJPEG's arithmetic
    op by op in fp32 (pad, colour tensordot, avg_pool2d, block split, the two 64-term tensordots per component, table division, round,
    and the way back).  The two alternate call by call in one process; each call is bracketed by device events; median and minimum of the
    per-call times after the warm-up, each route's peak memory above what is resident between calls, and the host time of a PIL JPEG
    encode + decode of the same B images (what ``jpeg_backend: pil`` does per sample)."""
    import io
    import itertools
    import math
    import statistics
    import time

    import numpy as np
    import torch.nn.functional as F
    from PIL import Image

    from dcpt_amd import functional as DF

    g = torch.Generator(device=dev).manual_seed(1234)
    low = torch.rand((B, 3, S // 8, S // 8), generator=g, device=dev)
    x = (F.interpolate(low, size=(S, S), mode="bilinear", align_corners=False) + 0.04 * torch.randn((B, 3, S, S), generator=g, device=dev)).clamp(0, 1)
    q = torch.tensor([(10.0, 20.0, 30.0, 40.0)[i % 4] for i in range(B)], device=dev)

    luma = torch.tensor([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                         [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                         [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], dtype=torch.float32, device=dev).t().contiguous()
    chroma = torch.full((8, 8), 99.0, device=dev)
    chroma[:4, :4] = torch.tensor([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]], dtype=torch.float32, device=dev).t()
    to_ycc = torch.tensor([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], device=dev).t().contiguous()
    to_rgb = torch.tensor([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], device=dev).t().contiguous()
    shift = torch.tensor([0.0, 128.0, 128.0], device=dev)
    fwd4 = torch.zeros((8, 8, 8, 8))
    inv4 = torch.zeros((8, 8, 8, 8))
    for a, b, u, v in itertools.product(range(8), repeat=4):
        fwd4[a, b, u, v] = math.cos((2 * a + 1) * u * math.pi / 16) * math.cos((2 * b + 1) * v * math.pi / 16)
        inv4[a, b, u, v] = math.cos((2 * u + 1) * a * math.pi / 16) * math.cos((2 * v + 1) * b * math.pi / 16)
    fwd4, inv4 = fwd4.to(dev), inv4.to(dev)
    alpha = torch.tensor([1 / math.sqrt(2)] + [1.0] * 7)
    alpha2 = torch.outer(alpha, alpha).to(dev)

    def split(p):
        n, h, w = p.shape
        return p.view(n, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(n, -1, 8, 8)

    def merge(p, h, w):
        return p.view(p.shape[0], h // 8, w // 8, 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(p.shape[0], h, w)

    def torch_route(img, quality):
        n, _, h, w = img.shape
        factor = (torch.where(quality < 50, 5000.0 / quality, 200.0 - quality * 2) / 100.0).view(n, 1, 1, 1)
        hp, wp = h + (-h % 16), w + (-w % 16)
        im = F.pad(img, (0, wp - w, 0, hp - h)) * 255
        ycc = torch.tensordot(im.permute(0, 2, 3, 1), to_ycc, dims=1) + shift
        planes = ycc.permute(0, 3, 1, 2).clone()
        comps = [ycc[..., 0], F.avg_pool2d(planes[:, 1:2], 2).squeeze(1), F.avg_pool2d(planes[:, 2:3], 2).squeeze(1)]
        out = []
        for k, comp in enumerate(comps):
            table = (luma if k == 0 else chroma).expand(n, 1, 8, 8) * factor
            coef = (alpha2 * 0.25) * torch.tensordot(split(comp) - 128, fwd4, dims=2)
            deq = torch.round(coef / table) * table
            rec = 0.25 * torch.tensordot(deq * alpha2, inv4, dims=2) + 128
            out.append(merge(rec, hp // (1 if k == 0 else 2), wp // (1 if k == 0 else 2)))
        up = [out[0]] + [c.unsqueeze(-1).repeat(1, 1, 2, 2).view(n, hp, wp) for c in out[1:]]
        rgb = torch.tensordot(torch.stack(up, 3) + (-shift), to_rgb, dims=1).permute(0, 3, 1, 2)
        rgb = torch.min(255 * torch.ones_like(rgb), torch.max(torch.zeros_like(rgb), rgb)) / 255
        return rgb[:, :, :h, :w]

    routes = {"kernel": lambda: DF.diffjpeg(x, q), "torch": lambda: torch_route(x, q)}
    peaks, last = {}, {}

    def call(name):
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = routes[name]()
        e1.record()
        e1.synchronize()
        peaks[name] = max(peaks.get(name, 0), torch.cuda.max_memory_allocated(dev) - base)
        last[name] = y
        return e0.elapsed_time(e1)

    times = {n: [] for n in routes}
    with torch.no_grad():
        for i in range(warmup + steps):
            for n in routes:
                t = call(n)
                if i >= warmup:
                    times[n].append(t)
    diff = (last["kernel"] - last["torch"]).abs()
    hwc = (x.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).cpu().numpy()
    qs = [int(v) for v in q.tolist()]
    pil = []
    for _ in range(3):
        t0 = time.perf_counter()
        for im, qq in zip(hwc, qs):
            buf = io.BytesIO()
            Image.fromarray(im).save(buf, format="JPEG", quality=qq)
            buf.seek(0)
            np.asarray(Image.open(buf).convert("RGB"), dtype=np.float32)
        pil.append((time.perf_counter() - t0) * 1e3)
    return dict(workload=f"JPEG round trip, {B} x 3 x {S} x {S}, one quality per image (10 / 20 / 30 / 40): DiffJPEG(differentiable=False)",
                kernel_ms_median=round(statistics.median(times["kernel"]), 4), kernel_ms_min=round(min(times["kernel"]), 4),
                torch_ms_median=round(statistics.median(times["torch"]), 4), torch_ms_min=round(min(times["torch"]), 4),
                ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 2),
                kernel_peak_mb=round(peaks["kernel"] / 1e6, 1), torch_peak_mb=round(peaks["torch"] / 1e6, 1),
                pil_host_ms_min=round(min(pil), 2), pil_images=B,
                max_abs_diff=float(diff.max()), share_above_1e_3=float((diff > 1e-3).float().mean()), calls=steps, warmup=warmup,
                note="device events around each call, the two routes alternating in one process; peak memory of a call above what is "
                     "allocated between calls (the kernel route's is its output and the [B] quality tensor); the torch route is the "
                     "reference's fp32 op sequence; max_abs_diff / share_above_1e_3 compare the two routes' outputs (a coefficient the fp32 "
                     "route rounds the other way shows as a block-sized difference); pil_host_ms_min is one thread's encode + decode of "
                     "all B images, best of 3")


def run_degrade(dev, steps=20, warmup=3, B=16, S=256):
    """The two on-the-fly degradations of a B x 3 x S x S batch (dcpt_amd/csrc/degrade.hip), each against a torch route on the device; two
    result lines.  Demosaic (Malvar, fp32 path, the mosaic fused): ``dcpt_amd.functional.demosaic`` against the mask-multiply mosaic, a
    reflect pad, one ``conv2d`` with the four 5 x 5 kernels and strided assignment by site.  Line mask: ``dcpt_amd.functional.inpaint_lines``
    against the same int64 rule as broadcast tensor arithmetic over (B, 10, S, S).  The two routes of a pair alternate call by call in one
    process; each call is bracketed by device events; median and minimum of the per-call times after the warm-up, each route's peak
    memory above what is resident between calls."""
    import statistics

    import torch.nn.functional as F

    from dcpt_amd import functional as DF

    g = torch.Generator(device=dev).manual_seed(1234)
    low = torch.rand((B, 3, S // 8, S // 8), generator=g, device=dev)
    x = (F.interpolate(low, size=(S, S), mode="bilinear", align_corners=False) + 0.04 * torch.randn((B, 3, S, S), generator=g, device=dev)).clamp(0, 1)
    rows, cols = torch.arange(S, device=dev).view(S, 1) % 2, torch.arange(S, device=dev).view(1, S) % 2
    site = torch.stack([(rows == 0) & (cols == 0), rows != cols, (rows == 1) & (cols == 1)]).float()
    k = torch.zeros((4, 1, 5, 5), device=dev)   # kgrb, krbg0, its transpose, krbbr, in units of 1/16
    k[0, 0, 2, 2], k[1, 0, 2, 2], k[3, 0, 2, 2] = 8, 10, 12
    for a in (1, 3):
        k[0, 0, 2, a] = k[0, 0, a, 2] = 4
        k[1, 0, 2, a] = 8
        for b in (1, 3):
            k[1, 0, a, b], k[3, 0, a, b] = -2, 4
    for a in (0, 4):
        k[0, 0, 2, a] = k[0, 0, a, 2] = k[1, 0, 2, a] = -2
        k[1, 0, a, 2] = 1
        k[3, 0, 2, a] = k[3, 0, a, 2] = -3
    k[2] = k[1].transpose(1, 2)
    k = k / 16

    def torch_demosaic(img):
        cfa = (img * site).sum(1, keepdim=True)
        conv = F.conv2d(F.pad(cfa, (2, 2, 2, 2), mode="reflect"), k)
        rgb = cfa.repeat(1, 3, 1, 1)
        rgb[:, 1, 0::2, 0::2], rgb[:, 1, 1::2, 1::2] = conv[:, 0, 0::2, 0::2], conv[:, 0, 1::2, 1::2]
        rgb[:, 0, 0::2, 1::2], rgb[:, 0, 1::2, 0::2], rgb[:, 0, 1::2, 1::2] = conv[:, 1, 0::2, 1::2], conv[:, 2, 1::2, 0::2], conv[:, 3, 1::2, 1::2]
        rgb[:, 2, 0::2, 1::2], rgb[:, 2, 1::2, 0::2], rgb[:, 2, 0::2, 0::2] = conv[:, 2, 0::2, 1::2], conv[:, 1, 1::2, 0::2], conv[:, 3, 0::2, 0::2]
        return rgb

    lines = torch.randint(0, S + 1, (B, 10, 4), generator=g, device=dev, dtype=torch.int32)
    meta = torch.stack([torch.randint(5, 11, (B,), generator=g, device=dev), torch.randint(5, 11, (B,), generator=g, device=dev),
                        torch.arange(B, device=dev) % 2], dim=1).to(torch.int32)
    py, px = torch.arange(S, device=dev).view(1, 1, S, 1), torch.arange(S, device=dev).view(1, 1, 1, S)

    def torch_inpaint(img, ln, mt):
        ln = ln.long()
        x1, y1, x2, y2 = (ln[:, :, i].view(B, 10, 1, 1) for i in range(4))
        qx, qy, dx, dy = px - x1, py - y1, x2 - x1, y2 - y1
        a, seg = qx * dx + qy * dy, dx * dx + dy * dy
        t2 = (mt[:, 1].long() ** 2).view(B, 1, 1, 1)
        hit = torch.where(a <= 0, 4 * (qx * qx + qy * qy) <= t2,
                          torch.where(a >= seg, 4 * ((qx - dx) ** 2 + (qy - dy) ** 2) <= t2, 4 * (qx * dy - qy * dx) ** 2 <= t2 * seg))
        hit = hit & (torch.arange(10, device=dev).view(1, 10, 1, 1) < mt[:, 0].view(B, 1, 1, 1))
        mask = hit.any(1, keepdim=True)
        return torch.where(mask, mt[:, 2].float().view(B, 1, 1, 1), img.clamp(0, 1))

    pairs = {"demosaic": {"kernel": lambda: DF.demosaic(x), "torch": lambda: torch_demosaic(x)},
             "inpaint_lines": {"kernel": lambda: DF.inpaint_lines(x, lines, meta), "torch": lambda: torch_inpaint(x, lines, meta)}}
    what = {"demosaic": f"Bayer mosaic + Malvar demosaic, {B} x 3 x {S} x {S}, fp32 path",
            "inpaint_lines": f"line-mask inpainting degradation, {B} x 3 x {S} x {S}, 5-10 strokes 5-10 thick per image"}
    out = []
    for name, routes in pairs.items():
        peaks, last, times = {}, {}, {n: [] for n in routes}
        with torch.no_grad():
            for i in range(warmup + steps):
                for n, fn in routes.items():
                    torch.cuda.synchronize(dev)
                    base = torch.cuda.memory_allocated(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    last[n] = fn()
                    e1.record()
                    e1.synchronize()
                    peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated(dev) - base)
                    if i >= warmup:
                        times[n].append(e0.elapsed_time(e1))
        moved = 4 * x.numel() * (5 / 3 if name == "demosaic" else 2)   # demosaic reads 2 of 3 planes' lines (every other row of R and B)
        out.append(dict(workload=what[name], kernel_ms_median=round(statistics.median(times["kernel"]), 4),
                        kernel_ms_min=round(min(times["kernel"]), 4), torch_ms_median=round(statistics.median(times["torch"]), 4),
                        torch_ms_min=round(min(times["torch"]), 4),
                        ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 2),
                        kernel_gb_per_s_at_min=round(moved / (min(times["kernel"]) * 1e-3) / 1e9, 1),
                        kernel_peak_mb=round(peaks["kernel"] / 1e6, 1), torch_peak_mb=round(peaks["torch"] / 1e6, 1),
                        max_abs_diff=float((last["kernel"] - last["torch"]).abs().max()), calls=steps, warmup=warmup,
                        note="device events around each call (the op's host side included), the two routes alternating in one process; "
                             "peak memory of a call above what is allocated between calls; kernel_gb_per_s_at_min counts the bytes the "
                             "algorithm needs (one read of the lines touched, one write) over the fastest call"))
    return out


def run_noise(dev, steps=20, warmup=3, B=32, S=256):
    """Gaussian noise on a B x 3 x S x S batch with one sigma per image (dcpt_amd/csrc/noise.hip) and ``feed_data`` of a mixed batch; two
    result lines.  Line 1: ``dcpt_amd.functional.gaussian_noise`` against the torch route on the device (``gt + sigma / 255 * randn_like``)
    and the host route of PairedImageDenoiseDataset (``RandomState(i).normal`` over S x S x 3 plus the add, the B images on one thread,
    best of 3).  Line 2: ``BaseModel._lq_on_device`` on a mixed batch (B / 4 images of each of noise, JPEG, demosaic, inpainting; gt on
    the host, as a loader hands it over) against the same four ops on four separate B / 4-image batches.  The routes of a pair alternate
    call by call in one process; each call is bracketed by device events; median and minimum of the per-call times after the warm-up,
    each route's peak memory above what is resident between calls."""
    import statistics
    import time

    import numpy as np
    import torch.nn.functional as F

    from basicsr.models.base_model import BaseModel
    from dcpt_amd import functional as DF

    g = torch.Generator(device=dev).manual_seed(1234)
    low = torch.rand((B, 3, S // 8, S // 8), generator=g, device=dev)
    x = F.interpolate(low, size=(S, S), mode="bilinear", align_corners=False).clamp(0, 1)
    sig_host = torch.tensor([(15.0, 25.0, 50.0)[i % 3] for i in range(B)])
    sigma, key = sig_host.to(dev), torch.arange(B, dtype=torch.int64, device=dev) + (7 << 32)
    scale = (sigma / 255).view(-1, 1, 1, 1)

    def measure(routes):
        peaks, last, times, wall = {}, {}, {n: [] for n in routes}, {n: [] for n in routes}
        with torch.no_grad():
            for i in range(warmup + steps):
                for n, fn in routes.items():
                    torch.cuda.synchronize(dev)
                    base = torch.cuda.memory_allocated(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    last[n] = fn()
                    e1.record()
                    e1.synchronize()
                    t1 = time.perf_counter()
                    peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated(dev) - base)
                    if i >= warmup:
                        times[n].append(e0.elapsed_time(e1))
                        wall[n].append((t1 - t0) * 1e3)
        return peaks, last, times, wall

    peaks, last, times, _ = measure({"kernel": lambda: DF.gaussian_noise(x, sigma, key), "torch": lambda: x + scale * torch.randn_like(x)})
    xh = x.cpu().permute(0, 2, 3, 1).contiguous().numpy()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for i in range(B):
            hwc = xh[i].copy()
            hwc += np.random.RandomState(i).normal(0, float(sig_host[i]) / 255.0, hwc.shape)
        host.append((time.perf_counter() - t0) * 1e3)
    noise = (last["kernel"] - x) / scale
    moved = 8 * x.numel()
    kmin = min(times["kernel"])
    first = dict(workload=f"Gaussian noise, {B} x 3 x {S} x {S}, one sigma per image (15 / 25 / 50): gt + sigma / 255 * n",
                 kernel_ms_median=round(statistics.median(times["kernel"]), 4), kernel_ms_min=round(kmin, 4),
                 torch_ms_median=round(statistics.median(times["torch"]), 4), torch_ms_min=round(min(times["torch"]), 4),
                 ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 2),
                 host_ms_min=round(min(host), 2), host_ms_per_image=round(min(host) / B, 3),
                 kernel_gb_per_s_at_min=round(moved / (kmin * 1e-3) / 1e9, 1), kernel_gnormals_per_s_at_min=round(x.numel() / (kmin * 1e-3) / 1e9, 2),
                 kernel_peak_mb=round(peaks["kernel"] / 1e6, 1), torch_peak_mb=round(peaks["torch"] / 1e6, 1),
                 kernel_noise_mean=round(float(noise.mean()), 5), kernel_noise_std=round(float(noise.std()), 5), calls=steps, warmup=warmup,
                 note="device events around each call (the op's host side included), the two device routes alternating in one process; peak "
                      "memory of a call above what is allocated between calls; kernel_gb_per_s_at_min counts one read and one write of the "
                      "batch over the fastest call, to set against the HBM rate; host_ms_min is one thread's RandomState(i).normal + add for "
                      "all B images, best of 3; the three routes draw different streams: they agree in distribution, not in value")

    # feed_data of a mixed batch against four single-kind batches
    model = BaseModel(dict(num_gpu=1, is_train=False))
    n = B // 4
    gt = x.cpu()
    gi = torch.Generator().manual_seed(99)
    lines = torch.randint(0, S + 1, (n, 10, 4), generator=gi, dtype=torch.int32)
    meta = torch.stack([torch.randint(5, 11, (n,), generator=gi), torch.randint(5, 11, (n,), generator=gi), torch.arange(n) % 2], dim=1).to(torch.int32)
    own = [dict(noise_sigma=sig_host[:n].clone(), noise_key=torch.arange(n, dtype=torch.int64)),
           dict(jpeg_quality=torch.tensor([(10.0, 20.0, 30.0, 40.0)[i % 4] for i in range(n)])),
           dict(mosaic=torch.zeros(n, dtype=torch.int32)), dict(inpaint_lines=lines, inpaint_meta=meta)]
    kind = torch.tensor([1 + i % 4 for i in range(4 * n)], dtype=torch.int32)      # interleaved, as a shuffled loader hands them over
    mixed = dict(gt=gt[:4 * n], degrade_kind=kind)
    for d in own:
        mixed.update(d)
    single = [dict(gt=gt[:4 * n][kind == k + 1].contiguous(), **own[k]) for k in range(4)]
    peaks, last, times, wall = measure({"mixed": lambda: model._lq_on_device(mixed), "separate": lambda: [model._lq_on_device(d) for d in single]})
    same = all(torch.equal(last["mixed"][kind.to(dev) == k + 1], last["separate"][k]) for k in range(4))
    second = dict(workload=f"feed_data's lq of a mixed batch, {4 * n} x 3 x {S} x {S}: {n} each of noise, JPEG, demosaic, inpainting, gt from the host",
                  mixed_ms_median=round(statistics.median(times["mixed"]), 4), mixed_ms_min=round(min(times["mixed"]), 4),
                  separate_ms_median=round(statistics.median(times["separate"]), 4), separate_ms_min=round(min(times["separate"]), 4),
                  mixed_wall_ms_median=round(statistics.median(wall["mixed"]), 4), separate_wall_ms_median=round(statistics.median(wall["separate"]), 4),
                  mixed_peak_mb=round(peaks["mixed"] / 1e6, 1), separate_peak_mb=round(peaks["separate"] / 1e6, 1), rows_bit_identical=bool(same),
                  calls=steps, warmup=warmup,
                  note="mixed: one transfer of gt, then per kind index_select -> the kind's kernel -> index_copy_ into lq; separate: the same "
                       "four kernels on four batches of their own (four transfers, no gather or scatter); both include the pageable "
                       "host-to-device copy of gt; the wall times add the host side after the last launch")
    return [first, second]


def run_poisson(dev, steps=20, warmup=3, B=32, S=256):
    """Poisson (shot) noise on a B x 3 x S x S batch at scale 1 with one key per image, images with all 256 levels (dcpt_amd/csrc/noise.hip):
    ``dcpt_amd.functional.poisson_noise`` against the reference's expression restated in torch on the same device (the rounded copy, the
    per-image ``len(torch.unique(...))`` loop with its read-backs, ``torch.poisson``, the blend; colour noise only, as a call with
    ``gray_noise=0`` runs it), the two alternating call by call in one process; device events around each call, each route's peak memory
    above what is resident between calls.  The two kernels' own times come from the library's launch timing (dcpt_prof_enable) in a
    second, separate pass of ``steps`` calls.  One result line."""
    import ctypes as C
    import statistics

    import numpy as np
    import torch.nn.functional as F

    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    g = torch.Generator(device=dev).manual_seed(1234)
    low = torch.rand((B, 3, S // 8, S // 8), generator=g, device=dev)
    x = (F.interpolate(low, size=(S, S), mode="bilinear", align_corners=False) * 1.2 - 0.1).clamp(0, 1)
    x[:, 0, 0, :256] = torch.arange(256, device=dev) / 255.0   # (every level present, whatever the field above holds)
    x = ((x * 255.0).round() / 255.0).contiguous()             # 8-bit images, as a loader hands them over
    key = torch.arange(B, dtype=torch.int64, device=dev) + (9 << 32)

    def torch_route():
        img = torch.clamp((x * 255.0).round(), 0, 255) / 255.0
        vals_list = [len(torch.unique(img[i, :, :, :])) for i in range(B)]
        vals_list = [2 ** np.ceil(np.log2(vals)) for vals in vals_list]
        vals = img.new_tensor(vals_list).view(B, 1, 1, 1)
        out = torch.poisson(img * vals) / vals
        return x + (out - img) * 1.0

    peaks, last, times = {}, {}, {"kernel": [], "torch": []}
    routes = {"kernel": lambda: DF.poisson_noise(x, 1.0, key), "torch": torch_route}
    with torch.no_grad():
        for i in range(warmup + steps):
            for n, fn in routes.items():
                torch.cuda.synchronize(dev)
                base = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                last[n] = fn()
                e1.record()
                e1.synchronize()
                peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated(dev) - base)
                if i >= warmup:
                    times[n].append(e0.elapsed_time(e1))
        _, vals = DF.poisson_noise(x, 1.0, key, return_vals=True)
        lib = _lib.load()
        lib.dcpt_prof_enable(1)
        for _ in range(steps):
            DF.poisson_noise(x, 1.0, key)
        torch.cuda.synchronize(dev)
        rows = (C.c_double * (8 * 16))()
        nrows = lib.dcpt_prof_read(rows, 16)
        lib.dcpt_prof_enable(0)
    per = {int(rows[8 * j]): rows[8 * j + 5] / max(rows[8 * j + 4], 1.0) for j in range(nrows)}
    noise = {n: last[n] - x for n in routes}
    kmin = min(times["kernel"])
    return dict(workload=f"Poisson noise, {B} x 3 x {S} x {S}, scale 1, one key per image, 256 levels per image: gt + (Poisson(q vals) / vals - q)",
                kernel_ms_median=round(statistics.median(times["kernel"]), 4), kernel_ms_min=round(kmin, 4),
                torch_ms_median=round(statistics.median(times["torch"]), 4), torch_ms_min=round(min(times["torch"]), 4),
                ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 2),
                levels_kernel_ms_mean=round(per.get(1032, float("nan")), 4), sampler_kernel_ms_mean=round(per.get(1033, float("nan")), 4),
                kernel_gsamples_per_s_at_min=round(x.numel() / (kmin * 1e-3) / 1e9, 2),
                kernel_peak_mb=round(peaks["kernel"] / 1e6, 1), torch_peak_mb=round(peaks["torch"] / 1e6, 1),
                vals=sorted(set(vals.tolist())), mean_rate=round(float(x.mean()) * 256, 1),
                kernel_noise_mean=round(float(noise["kernel"].mean()), 6), kernel_noise_std=round(float(noise["kernel"].std()), 5),
                torch_noise_mean=round(float(noise["torch"].mean()), 6), torch_noise_std=round(float(noise["torch"].std()), 5),
                calls=steps, warmup=warmup,
                note="device events around each call (the op's host side included), the two routes alternating in one process; peak memory "
                     "of a call above what is allocated between calls; the torch route is the reference's expression for colour noise "
                     "(one torch.unique and one read-back per image, torch.poisson, the blend); levels / sampler_kernel_ms_mean are the "
                     "library's per-launch event timing over a separate pass of `calls` calls; the two routes draw different streams: "
                     "they agree in distribution (the noise mean and std of both are given), not in value")


def run_blur(dev, steps=20, warmup=3, B=32, S=256, K=21):
    """Synthetic blur of a B x 3 x S x S batch with one K x K kernel per image (dcpt_amd/csrc/blur.hip): ``dcpt_amd.functional.filter2d``
    against the reference's form on the same device (``F.pad(mode="reflect")`` plus ``F.conv2d`` with B * 3 groups and the kernels repeated
    over the channels), the two alternating call by call in one process, device events around each call, each route's peak memory above what
    is resident between calls; ``USMSharp`` at radius 50 (two 51 x 51 blurs and the element-wise steps) the same way on its own; and
    ``basicsr.data.filter2d_host`` over the B images on one host thread (one pass).  One result line.  The fp64 rate counts the kernel's
    own 2 K^2 B C H W flops over its fastest call."""
    import statistics
    import time

    import torch.nn.functional as F

    from basicsr.data import filter2d_host
    from basicsr.data.degradations import random_mixed_kernels
    from basicsr.utils import USMSharp
    from dcpt_amd import functional as DF

    import random

    import numpy as np

    g = torch.Generator(device=dev).manual_seed(1234)
    low = torch.rand((B, 3, S // 8, S // 8), generator=g, device=dev)
    x = (F.interpolate(low, size=(S, S), mode="bilinear", align_corners=False) + 0.05 * torch.randn((B, 3, S, S), generator=g, device=dev)).clamp(0, 1)
    rng = (random.Random(77), np.random.RandomState(77))
    kinds = ["iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso"]
    kern_host = torch.from_numpy(np.stack([random_mixed_kernels(kinds, [1 / 6] * 6, K, (0.2, 3), (0.2, 3), rng=rng) for _ in range(B)]).astype(np.float32))
    kern = kern_host.to(dev)

    def torch_route():
        r = K // 2
        p = F.pad(x, (r, r, r, r), mode="reflect")
        w = kern.view(B, 1, K, K).repeat(1, 3, 1, 1).view(B * 3, 1, K, K)
        return F.conv2d(p.view(1, B * 3, S + 2 * r, S + 2 * r), w, groups=B * 3).view(B, 3, S, S)

    def measure(routes):
        peaks, last, times = {}, {}, {n: [] for n in routes}
        with torch.no_grad():
            for i in range(warmup + steps):
                for n, fn in routes.items():
                    torch.cuda.synchronize(dev)
                    base = torch.cuda.memory_allocated(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    last[n] = fn()
                    e1.record()
                    e1.synchronize()
                    peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated(dev) - base)
                    if i >= warmup:
                        times[n].append(e0.elapsed_time(e1))
        return peaks, last, times

    peaks, last, times = measure({"kernel": lambda: DF.filter2d(x, kern), "torch": torch_route})
    diff = float((last["kernel"].double() - last["torch"].double()).abs().max())
    usm = USMSharp(50).to(dev)
    upeaks, _, utimes = measure({"usm": lambda: usm(x)})
    xh = x.cpu()
    t0 = time.perf_counter()
    host0 = None
    for i in range(B):
        lq = filter2d_host(xh[i], kern_host[i])
        host0 = lq if host0 is None else host0
    host_ms = (time.perf_counter() - t0) * 1e3
    same = bool(torch.equal(host0.view(torch.int32), last["kernel"][0].cpu().view(torch.int32)))
    kmin, umin = min(times["kernel"]), min(utimes["usm"])
    flops = 2.0 * K * K * x.numel()
    return dict(workload=f"synthetic blur, {B} x 3 x {S} x {S}, one {K} x {K} kernel per image: filter2D",
                kernel_ms_median=round(statistics.median(times["kernel"]), 4), kernel_ms_min=round(kmin, 4),
                torch_ms_median=round(statistics.median(times["torch"]), 4), torch_ms_min=round(min(times["torch"]), 4),
                ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 2),
                kernel_fp64_tflops_at_min=round(flops / (kmin * 1e-3) / 1e12, 2),
                kernel_peak_mb=round(peaks["kernel"] / 1e6, 1), torch_peak_mb=round(peaks["torch"] / 1e6, 1),
                kernel_vs_torch_max_abs=float(f"{diff:.3e}"), host_row0_bit_identical=same,
                usm_radius50_ms_median=round(statistics.median(utimes["usm"]), 4), usm_radius50_ms_min=round(umin, 4),
                usm_fp64_tflops_at_min=round(2 * 2.0 * 51 * 51 * x.numel() / (umin * 1e-3) / 1e12, 2), usm_peak_mb=round(upeaks["usm"] / 1e6, 1),
                host_ms=round(host_ms, 1), host_ms_per_image=round(host_ms / B, 2), calls=steps, warmup=warmup,
                note="device events around each call (the op's host side included), filter2d and the torch form (F.pad reflect + F.conv2d "
                     "with B * C groups, the kernels repeated over the channels) alternating in one process; peak memory of a call above "
                     "what is allocated between calls; kernel_fp64_tflops_at_min = 2 K^2 B C H W flops over the fastest call (the usm figure "
                     "counts its two 51 x 51 blurs over the whole forward, element-wise steps included); host_ms is filter2d_host (numpy "
                     "float64, the kernel's tap order) over the B images on one thread, one pass")


def run_degrade_chain(dev, steps=20, warmup=3, B=32, S=256, scale=4):
    """The resize kernel and the second-order degradation chain on a B x 3 x S x S batch (dcpt_amd/csrc/resize.hip,
    basicsr/data/degradations.py).  Line 1: ``dcpt_amd.functional.interpolate`` per mode at the scale factors 1.5, 0.5 and 0.15 against
    ``F.interpolate`` (fp32) on the same device, the two alternating call by call, device events around each call.  Line 2:
    ``apply_second_order`` over eight seeded plans of the shipped options (options/realsr/train_SwinIR_realSR_x4.yml) against the same
    chain with ``F.interpolate`` in place of the kernel, alternating plan by plan, and each route's peak memory above what is resident
    between calls.  The bandwidth figure counts one read of the source and one write of the result over the kernel's fastest call."""
    import random
    import statistics

    import numpy as np
    import torch.nn.functional as F

    from basicsr.data import degradations as D
    from dcpt_amd import functional as DF

    g = torch.Generator(device=dev).manual_seed(1234)
    low = torch.rand((B, 3, S // 8, S // 8), generator=g, device=dev)
    x = (F.interpolate(low, size=(S, S), mode="bilinear", align_corners=False) + 0.05 * torch.randn((B, 3, S, S), generator=g, device=dev)).clamp(0, 1)

    def torch_interp(x, size=None, scale_factor=None, mode="bilinear", clip=False, rounds=False):
        return F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode, **({} if mode == "area" else {"align_corners": False}))

    def measure(routes, calls):
        peaks, last, times = {}, {}, {n: [] for n in routes}
        with torch.no_grad():
            for i in range(warmup + calls):
                for n, fn in routes.items():
                    torch.cuda.synchronize(dev)
                    base = torch.cuda.memory_allocated(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    last[n] = fn(i)
                    e1.record()
                    e1.synchronize()
                    peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated(dev) - base)
                    if i >= warmup:
                        times[n].append(e0.elapsed_time(e1))
        return peaks, last, times

    per_mode = {}
    for mode in DF.INTERP_MODES:
        for sf in (1.5, 0.5, 0.15):
            peaks, last, times = measure({"kernel": lambda i: DF.interpolate(x, scale_factor=sf, mode=mode),
                                          "torch": lambda i: torch_interp(x, scale_factor=sf, mode=mode)}, steps)
            kmin = min(times["kernel"])
            per_mode[f"{mode}@{sf}"] = dict(
                out=list(last["kernel"].shape[2:]), kernel_ms_median=round(statistics.median(times["kernel"]), 4), kernel_ms_min=round(kmin, 4),
                torch_ms_median=round(statistics.median(times["torch"]), 4), torch_ms_min=round(min(times["torch"]), 4),
                ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 2),
                kernel_gb_s_at_min=round(4.0 * (x.numel() + last["kernel"].numel()) / (kmin * 1e-3) / 1e9, 1),
                kernel_vs_torch_max_abs=float(f"{float((last['kernel'] - last['torch']).abs().max()):.3e}"))
    first = dict(workload=f"interpolate, {B} x 3 x {S} x {S}, per mode at scale_factor 1.5 / 0.5 / 0.15 (ratios 1/1.5, 1/0.5, 1/0.15), against F.interpolate fp32",
                 results=per_mode, calls=steps, warmup=warmup,
                 note="device events around each call (the op's host side included), the kernel and F.interpolate alternating in one process; "
                      "kernel_gb_s_at_min = 4 bytes x (source + result elements) over the fastest call")

    opt = dict(resize_prob=[0.2, 0.7, 0.1], resize_range=[0.15, 1.5], gaussian_noise_prob=0.5, noise_range=[1, 30], poisson_scale_range=[0.05, 3],
               gray_noise_prob=0.4, jpeg_range=[30, 95], second_blur_prob=0.8, resize_prob2=[0.3, 0.4, 0.3], resize_range2=[0.3, 1.2],
               gaussian_noise_prob2=0.5, noise_range2=[1, 25], poisson_scale_range2=[0.05, 2.5], gray_noise_prob2=0.4, jpeg_range2=[30, 95])
    rng = (random.Random(77), np.random.RandomState(77))
    kinds = ["iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso"]
    kernels = [torch.from_numpy(np.stack([D.random_mixed_kernels(kinds, [0.45, 0.25, 0.12, 0.03, 0.12, 0.03], 21, (0.2, 3), (0.2, 3), rng=rng)
                                          for _ in range(B)]).astype(np.float32)).to(dev) for _ in range(3)]
    plans = [D.draw_second_order_plan(opt, B, S, S, scale, rng=rng) for _ in range(8)]

    def chain(interp):
        def run(i):
            saved, DF.interpolate = DF.interpolate, interp
            try:
                return D.apply_second_order(x, *kernels, plans[i % len(plans)])
            finally:
                DF.interpolate = saved
        return run

    calls = max(steps, 2 * len(plans))
    peaks, last, times = measure({"kernel": chain(DF.interpolate), "torch": chain(torch_interp)}, calls)
    second = dict(workload=f"second-order degradation chain, {B} x 3 x {S} x {S} -> x{scale}, eight seeded plans of the shipped options: apply_second_order",
                  kernel_ms_median=round(statistics.median(times["kernel"]), 4), kernel_ms_min=round(min(times["kernel"]), 4),
                  torch_ms_median=round(statistics.median(times["torch"]), 4), torch_ms_min=round(min(times["torch"]), 4),
                  ratio_median=round(statistics.median(times["torch"]) / statistics.median(times["kernel"]), 3),
                  kernel_peak_mb=round(peaks["kernel"] / 1e6, 1), torch_peak_mb=round(peaks["torch"] / 1e6, 1),
                  lq_max_abs_between_routes=float(f"{float((last['kernel'] - last['torch']).abs().max()):.3e}"),
                  plans=[dict(resize1=[round(p["resize1"]["scale_factor"], 3), p["resize1"]["mode"]], noise1=p["noise1"]["kind"],
                              second_blur=p["second_blur"], resize2=[list(p["resize2"]["size"]), p["resize2"]["mode"]], noise2=p["noise2"]["kind"],
                              final_first=p["final_first"], final_mode=p["final_mode"]) for p in plans],
                  calls=calls, warmup=warmup,
                  note="device events around each call, host side of the ops and the plan's small host-to-device copies included; the two routes "
                       "alternate and see the same plan in the same call; `torch` is the same chain with F.interpolate (fp32) in place of "
                       "dcpt_amd.functional.interpolate; peak memory of a call above what is allocated between calls; the routes' lq may "
                       "differ by grid steps where a JPEG coefficient or the final rounding sits next to a tie")
    return [first, second]


def run_knn(dev, steps=20, warmup=3, N=500, D=524288, classes=5, k=5):
    """The kNN degradation probe at the reference's size (basicsr/utils/knn_probe.py, dcpt_amd/csrc/knn.hip): N seeded fp32 rows of D values
    (a NAFNet-32 last decoder map at 128 x 128) in ``classes`` clusters, the reference's five seeded 67/33 splits.  Routes, alternating call
    by call in one process with device events around each call: ``pairwise_sqdist`` (the fp64 MFMA kernels) and then ``knn_vote`` over the
    five splits; ``torch.cdist`` of the rows cast to fp64 plus ``topk`` per split on the device.  ``knn_probe`` end to end (split rule,
    kernels, the one transfer, the reports) and, where it is installed, scikit-learn's ``KNeighborsClassifier(5)`` on 16 host threads
    (one pass over the five splits, wall time) are timed on their own.  The fp64 rate counts 2 N^2 D flops over the fastest call."""
    import statistics
    import time

    import numpy as np

    from basicsr.utils import knn_probe, train_test_indices
    from basicsr.utils.knn_probe import KNN_SEEDS
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    g = torch.Generator(device=dev).manual_seed(1234)
    labels = np.arange(N) % classes + 1
    centres = torch.randn((classes, D), generator=g, device=dev)
    x = torch.randn((N, D), generator=g, device=dev)
    x += 0.05 * centres[torch.from_numpy(labels - 1).to(dev)]
    del centres
    splits = [train_test_indices(N, 0.33, s) for s in KNN_SEEDS]
    train = torch.from_numpy(np.stack([tr for tr, _ in splits])).to(dev)
    test = torch.from_numpy(np.stack([te for _, te in splits])).to(dev)
    lab_dev = torch.from_numpy(labels).to(dev)
    d2 = torch.empty((N, N), dtype=torch.float64, device=dev)

    def kernel_route():
        DF.pairwise_sqdist(x, out=d2)
        return DF.knn_vote(d2, lab_dev, train, test, k)[0]

    def torch_route():
        x64 = x.double()
        dist = torch.cdist(x64, x64)
        return torch.stack([dist[test[s]][:, train[s]].topk(k, dim=1, largest=False).indices for s in range(len(splits))])

    routes = {"kernel": kernel_route, "pdist2": lambda: DF.pairwise_sqdist(x, out=d2), "torch": torch_route}
    peaks, last, times = {}, {}, {n: [] for n in routes}
    with torch.no_grad():
        for i in range(warmup + steps):
            for n, fn in routes.items():
                torch.cuda.synchronize(dev)
                base = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                last[n] = fn()
                e1.record()
                e1.synchronize()
                peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated(dev) - base)
                if i >= warmup:
                    times[n].append(e0.elapsed_time(e1))

    def votes(nbr_labels):   # (largest count, smallest label): the rule of dcpt_knn_vote_fwd
        out = np.empty(nbr_labels.shape[:-1], dtype=np.int64)
        for idx in np.ndindex(*out.shape):
            vals, counts = np.unique(nbr_labels[idx], return_counts=True)
            out[idx] = vals[np.argmax(counts)]
        return out

    pred_kernel = last["kernel"].cpu().numpy()
    train_h = train.cpu().numpy()
    pred_torch = votes(np.stack([labels[train_h[s][last["torch"][s].cpu().numpy()]] for s in range(len(splits))]))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    reports, mean_acc = knn_probe(x, labels)
    probe_ms = (time.perf_counter() - t0) * 1e3
    lib = _lib.load()
    nws = lib.dcpt_pdist2_ws_bytes(N, N, D, 0)
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    ksplit = next((c for c in range(1, 65536) if al(8 * c * N * N) + 2 * al(8 * c * N) == nws), None)
    res = dict(workload=f"kNN degradation probe: {N} fp32 rows of {D} values, {classes} labels, k = {k}, five seeded 67/33 splits",
               pdist2_ms_median=round(statistics.median(times["pdist2"]), 3), pdist2_ms_min=round(min(times["pdist2"]), 3),
               pdist2_fp64_tflops_at_min=round(2.0 * N * N * D / (min(times["pdist2"]) * 1e-3) / 1e12, 2), fp64_matrix_peak_tflops_published=78.6,
               pdist2_plus_vote_ms_median=round(statistics.median(times["kernel"]), 3),
               torch_cdist_fp64_topk_ms_median=round(statistics.median(times["torch"]), 3), torch_cdist_fp64_topk_ms_min=round(min(times["torch"]), 3),
               knn_probe_end_to_end_ms=round(probe_ms, 2), mean_accuracy=round(mean_acc, 4), ksplit_chosen=ksplit, workspace_mb=round(nws / 1e6, 1),
               kernel_peak_mb=round(peaks["kernel"] / 1e6, 1), torch_peak_mb=round(peaks["torch"] / 1e6, 1),
               predictions_differing_kernel_vs_torch=int((pred_kernel != pred_torch).sum()), predictions=int(pred_kernel.size),
               probe_vs_kernel_route_differing=int(sum((r["pred"] != pred_kernel[s]).sum() for s, r in enumerate(reports))),
               calls=steps, warmup=warmup,
               note="device events around each call, the routes alternating in one process; pdist2 = pairwise_sqdist alone (norm, MFMA and "
                    "finishing launches), kernel route = pairwise_sqdist + knn_vote over the five splits, torch route = the rows cast to fp64, "
                    "torch.cdist and topk per split; peak memory of a call above what is allocated between calls; knn_probe_end_to_end_ms is one "
                    "wall-clock call with the transfer and the host reports")
    try:
        from sklearn.neighbors import KNeighborsClassifier
    except ImportError:
        res["sklearn"] = "not installed"
        return res
    xh = x.cpu().numpy()
    t0 = time.perf_counter()
    pred_sk = np.stack([KNeighborsClassifier(n_neighbors=k, n_jobs=16).fit(xh[tr], labels[tr]).predict(xh[te]) for tr, te in splits])
    res.update(sklearn_16_threads_ms=round((time.perf_counter() - t0) * 1e3, 1), predictions_differing_kernel_vs_sklearn=int((pred_kernel != pred_sk).sum()))
    return res


def run_tsne(dev, sizes=(500, 4096), D=64, classes=5, max_iter=2000):
    """Exact t-SNE on the device (basicsr/utils/tsne.py, dcpt_amd/csrc/tsne.hip) at the kNN workload's row count and at 4096 rows: seeded
    blobs of D values in ``classes`` clusters, unit-length rows, perplexity 30, the full ``max_iter``-iteration schedule from the "random"
    start (wall time of ``tsne_embed`` on the resident distance matrix, with its read-back every 50 iterations).  Next to it: the
    affinities alone; 50 iterations in one ``tsne_steps`` call and the same 50 written as float64 torch expressions on the same device
    (device events, alternating, median of 5 after 1 warm-up); where scikit-learn is installed ``TSNE(method="exact")`` and the default
    Barnes-Hut on the host (wall time, one run; the exact method at more than 1000 rows for 250 iterations only).  One dict per size."""
    import statistics
    import time

    import numpy as np

    from basicsr.utils import neighbour_label_share, tsne_embed
    from dcpt_amd import functional as DF

    EPS = 2.0 ** -52

    def torch_steps(P, Y, update, gains, n, ex, mom, lr):
        Pe = ex * P
        for _ in range(n):
            diff = Y[:, None, :] - Y[None, :, :]
            w = 1.0 / (1.0 + (diff * diff).sum(-1))
            w.fill_diagonal_(0.0)
            Q = torch.clamp_min(w / w.sum(), EPS)
            g = 4.0 * (((Pe - Q) * w)[:, :, None] * diff).sum(1)
            gains = torch.clamp_min(torch.where(update * g < 0.0, gains + 0.2, gains * 0.8), 0.01)
            update = mom * update - lr * (g * gains)
            Y = Y + update
        return Y

    out = []
    for N in sizes:
        rs = np.random.RandomState(1234)
        labels = np.arange(N) % classes
        X = (10.0 * rs.standard_normal((classes, D))[labels] + rs.standard_normal((N, D))).astype(np.float32)
        x = torch.from_numpy(X).to(dev)
        x = x / x.norm(dim=1, keepdim=True)
        d2 = DF.pairwise_sqdist(x)
        lr = max(N / 12.0 / 4.0, 50.0)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            r = fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), r

        aff = [timed(lambda: DF.tsne_affinities(d2, 30.0)) for _ in range(4)]
        P = aff[-1][1][0]
        Y0 = torch.from_numpy(1e-4 * np.random.RandomState(0).standard_normal((N, 2))).to(dev)
        t_kernel, t_torch = [], []
        for i in range(6):
            Y, u, g = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
            tk, _ = timed(lambda: DF.tsne_steps(P, Y, u, g, 50, 12.0, 0.5, lr))
            tt, Yt = timed(lambda: torch_steps(P, Y0, torch.zeros_like(Y0), torch.ones_like(Y0), 50, 12.0, 0.5, lr))
            if i:
                t_kernel.append(tk / 50)
                t_torch.append(tt / 50)
        agree = float((Y - Yt).abs().max() / Yt.abs().max())
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        res = tsne_embed(d2=d2, max_iter=max_iter, init="random")
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated(dev) - base
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        torch_steps(P, Y0, torch.zeros_like(Y0), torch.ones_like(Y0), 1, 12.0, 0.5, lr)
        torch.cuda.synchronize(dev)
        peak_torch = torch.cuda.max_memory_allocated(dev) - base
        line = dict(workload=f"exact t-SNE of {N} unit-length rows ({D} values, {classes} blobs), perplexity 30, {max_iter} iterations, random start",
                    affinities_ms_median=round(statistics.median(t for t, _ in aff[1:]), 3),
                    schedule_wall_s=round(wall, 3), schedule_ms_per_iteration=round(wall * 1e3 / (res["n_iter"] + 1), 4), n_iter=res["n_iter"],
                    kl_divergence=round(res["kl_divergence"], 6), neighbour_label_share=neighbour_label_share(res["embedding"], labels, 5),
                    steps50_kernel_ms_per_iteration_median=round(statistics.median(t_kernel), 4),
                    steps50_kernel_ms_per_iteration_min=round(min(t_kernel), 4),
                    steps50_torch_fp64_ms_per_iteration_median=round(statistics.median(t_torch), 4),
                    steps50_torch_fp64_ms_per_iteration_min=round(min(t_torch), 4),
                    kernel_vs_torch_after_50_steps_rel=agree, schedule_peak_mb_above_inputs=round(peak / 1e6, 1),
                    torch_step_peak_mb_above_inputs=round(peak_torch / 1e6, 1),
                    note="schedule = tsne_embed on the resident distance matrix: affinities, the descent in chunks of 50 with one read-back of two "
                         "numbers per chunk, the final KL and the transfer of the embedding, wall clock; steps50 = device events around 50 "
                         "iterations, the two routes alternating, 5 timed after 1 warm-up; peak memory of a call above what is allocated before "
                         "it (for the schedule that includes P, N^2 doubles)")
        try:
            from sklearn.manifold import TSNE
        except ImportError:
            line["sklearn"] = "not installed"
            out.append(line)
            continue
        xh = x.cpu().numpy()
        it_exact = max_iter if N <= 1000 else 250
        for key, kw, its in (("sklearn_exact", dict(method="exact"), it_exact), ("sklearn_barnes_hut", dict(), max_iter)):
            print(f"tsne N={N}: {key}, {its} iterations on the host ...", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            ts = TSNE(n_components=2, max_iter=its, init="random", random_state=0, **kw)
            Ys = ts.fit_transform(xh)
            dt = time.perf_counter() - t0
            line.update({f"{key}_wall_s": round(dt, 2), f"{key}_iterations": int(ts.n_iter_) + 1,
                         f"{key}_ms_per_iteration": round(dt * 1e3 / (int(ts.n_iter_) + 1), 3), f"{key}_kl": round(float(ts.kl_divergence_), 6) if ts.kl_divergence_ < 1e300 else None,   # (max_iter = 250: scikit-learn's second phase is empty and its error stays at the float maximum)
                         f"{key}_neighbour_label_share": neighbour_label_share(Ys, labels, 5)})
        out.append(line)
    return out


def run_niqe(dev, steps=20, warmup=3, H=1080, W=2048):
    """NIQE of one 1 x 3 x H x W image (a smooth random field plus fine noise, no flat block): the host ``calculate_niqe`` (numpy float64,
    one thread's wall time, best of 2) against ``calculate_niqe_device`` (the fused fp64 kernels of dcpt_amd/csrc/niqe.hip + the host
    finish; device events around each whole call, which ends with the one transfer and the 36 x 36 algebra) and against the launches
    alone (dcpt_amd.functional.niqe_stats).  The pristine model is read from DCPT_NIQE_PRIS_PARAMS, else tests/golden."""
    import statistics

    from basicsr.metrics import calculate_niqe, calculate_niqe_device
    from dcpt_amd import functional as DF

    pris = os.environ.get("DCPT_NIQE_PRIS_PARAMS") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden",
                                                                    "niqe_pris_params.npz")
    g = torch.Generator().manual_seed(19)
    low = torch.rand((1, 3, H // 16, W // 16), generator=g) * 0.5 + 0.25
    img = (torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
           + 0.02 * torch.randn((1, 3, H, W), generator=g)).clamp(0, 1)
    x = img.to(dev)
    host_ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        host = calculate_niqe(img.numpy(), 0, pris_params=pris)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    routes = {"device": lambda: calculate_niqe_device(x, 0, pris_params=pris), "launches": lambda: DF.niqe_stats(x, 0)}
    peaks, last, times = {}, {}, {n: [] for n in routes}
    for i in range(warmup + steps):
        for n, fn in routes.items():
            torch.cuda.synchronize(dev)
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[n] = fn()
            e1.record()
            e1.synchronize()
            peaks[n] = max(peaks.get(n, 0), torch.cuda.max_memory_allocated(dev) - base)
            if i >= warmup:
                times[n].append(e0.elapsed_time(e1))
    return dict(workload=f"NIQE of one 1 x 3 x {H} x {W} image, crop_border 0",
                host_ms_min=round(min(host_ms), 1), device_ms_median=round(statistics.median(times["device"]), 3),
                device_ms_min=round(min(times["device"]), 3), launches_ms_median=round(statistics.median(times["launches"]), 4),
                launches_ms_min=round(min(times["launches"]), 4), device_peak_mb=round(peaks["device"] / 1e6, 1),
                niqe_host=host, niqe_device=last["device"], rel_diff=abs(host - last["device"]) / abs(host), calls=steps, warmup=warmup,
                note="device events around each call; device_ms is calculate_niqe_device whole (six launches, the one transfer of the "
                     "[3][231][2][5][6] sums, the numpy finish), launches_ms the six launches alone without a synchronisation inside; "
                     "peak memory of a call above the resident image (MSCN plane, x0.5 image, resize intermediate in the workspace, "
                     "sums); host_ms_min is numpy float64 on one thread's wall clock, best of 2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=["dcpt", "dcpt_swinir", "restormer", "promptir", "infer2k", "naf", "swinir", "rcan", "val_metrics", "val_metrics_ms", "step_tail", "tlsc", "ssim_loss", "ldl", "jpeg", "niqe", "degrade", "noise", "blur", "poisson", "degrade_chain", "knn", "tsne"])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "bf16_tail32", "bf16_edge32", "bf16_res32"])
    ap.add_argument("--head-dtype", default=None, choices=["fp32", "bf16"], help="dcpt: classifier-head activations (default: --dtype)")
    ap.add_argument("--restormer-save", default="balanced", choices=["auto", "lean", "balanced", "full"], help="what the Restormer halves keep for backward")
    ap.add_argument("--optimizer", default="dcpt", choices=["dcpt", "torch"], help="A/B: torch = torch.optim.AdamW(fused=True) instead of dcpt_amd.optim.FusedAdamW")
    ap.add_argument("--two-pass", action="store_true", help="dcpt A/B: train.batched_encoder_passes false (the reference's two encoder passes, B each, instead of one pass over 2B)")
    ap.add_argument("--torch-taps", action="store_true", help="dcpt_swinir A/B: the strided taps as torch indexing (feature[:, :, ::s, ::s] into the dense "
                    "mix: a gather copy forward; a zero fill, a strided scatter and a full-map add backward) instead of dcpt_mix_stride_* / dcpt_grid_add")
    ap.add_argument("--upsampler", default="", choices=["", "pixelshuffle", "pixelshuffledirect", "nearest+conv"], help="swinir: super-resolution tail")
    ap.add_argument("--upscale", type=int, default=1, help="swinir: scale of --upsampler")
    ap.add_argument("--grad-clip", type=float, default=0.0, help="restormer: clip_grad_norm_ before the optimizer step (grad_clip of the YAML)")
    ap.add_argument("--ema-decay", type=float, default=0.0, help="restormer: EMA copy of the parameters updated after the step (train.ema_decay)")
    ap.add_argument("--fused-step-tail", action="store_true", help="restormer: clip + step + EMA as the one call of train.fused_step_tail")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tile-streams", type=int, default=2, help="infer2k: HIP streams the tile batches run on (tile.streams)")
    ap.add_argument("--tile", type=int, default=0, help="tlsc: 0 = the whole 1080 x 2048 image in one forward, else test_tile's infer_size (tile_pad 16)")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--side-stream", type=int, default=1, choices=[0, 1], help="0: weight-gradient work on the caller's stream (serialized kernel times)")
    ap.add_argument("--gpus", type=int, default=1, help="dcpt / restormer: data-parallel ranks, one process per GPU over RCCL (same protocol as bench.py: "
                                                        "self-spawns under torch.distributed.run, barrier + max over ranks, rccl_ranks on the line)")
    ap.add_argument("--path-check-shared-device", action="store_true",
                    help="PATH CHECK ONLY, never a measurement: the ranks share the visible GPU(s), collectives over gloo (the line is marked invalid)")
    args = ap.parse_args()
    if args.gpus > 1 and args.workload not in ("dcpt", "restormer"):
        raise SystemExit("--gpus N: data-parallel lines exist for the training workloads dcpt (configs[2]) and restormer (configs[3])")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        import bench

        if torch.cuda.device_count() < args.gpus and not args.path_check_shared_device:
            raise SystemExit(f"--gpus {args.gpus} but only {torch.cuda.device_count()} device(s) visible on this node")
        if args.path_check_shared_device:   # (spawn_ranks refuses more ranks than devices: the shared-device check launches its ranks itself)
            import socket
            import subprocess

            with socket.socket() as sock:
                sock.bind(("127.0.0.1", 0))
                port = sock.getsockname()[1]
            raise SystemExit(subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
                                              "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]))
        return bench.spawn_ranks(args.gpus, script=os.path.abspath(__file__))
    if args.dtype == "bf16_res32" and args.workload not in ("rcan", "swinir"):
        raise SystemExit("--dtype bf16_res32: the fp32 residual stream exists for --workload rcan and swinir")
    rank, local_rank, world = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    local_rank %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group(backend="gloo") if args.path_check_shared_device else dist.init_process_group(backend="nccl", device_id=dev)
    if not args.side_stream:
        from dcpt_amd import _lib

        _lib.load().dcpt_set_side_stream(0)
    from basicsr.archs import build_network
    from dcpt_amd.keyed_init import fill_module_

    if args.optimizer == "torch":   # A/B of the optimizer step: torch's fused kernel behind the same constructor
        import dcpt_amd.optim as _O

        _O.FusedAdamW = lambda params, lr=1e-3, **kw: torch.optim.AdamW(params, lr, **{**kw, "fused": True})
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    bf = args.dtype.startswith("bf16")
    naf = dict(NAF, act_dtype=args.dtype)
    # SURVEY 8d algorithmic HBM bytes of NAFNet-64 fwd+bwd per 256^2 image: 25 element passes over the blocks' sum c*P = 30.146 M
    # + 3 passes over the 40.4 M elements of the layers between the groups; 4 B per element in fp32, 2 B in bf16 storage (end to end)
    naf_bytes = (25 * 30.146e6 + 3 * 40.4e6) * (2 if bf else 4)
    peak = 2.5e15 if bf else 157.3e12

    def rooflines(flops, nbytes, dt):
        return dict(alg_tflops=round(flops / dt / 1e12, 2), mfma_peak_tflops=peak / 1e12, mfma_frac=round(flops / dt / peak, 4),
                    alg_gbytes=round(nbytes / 1e9, 2), hbm_frac=round(nbytes / dt / 8e12, 4),
                    bound="hbm" if nbytes / 8e12 > flops / peak else "mfma",
                    note="hbm_frac against the 8 TB/s spec roof; a streaming kernel reaches ~6.3 TB/s (0.79) on this part")

    if args.workload == "naf":
        # configs[1]'s network and batch, as a bf16-vs-fp32 comparison line (the fp32 headline is bench.py's, never this one)
        B, S = args.batch or 32, args.size or 256
        net = fill_module_(build_network(dict(type="NAFNetBaseline", **naf))).to(dev)
        from dcpt_amd.optim import FusedAdamW

        optm = FusedAdamW(net.parameters(), lr=1e-4, betas=(0.9, 0.9), weight_decay=0.0)
        lq = torch.rand((B, 3, S, S), generator=g, device=dev)
        gt = torch.rand((B, 3, S, S), generator=g, device=dev)

        def step():
            optm.zero_grad(set_to_none=True)
            (net(lq) - gt).abs().mean().backward()
            optm.step()

        dt = timed(step, args.steps, args.warmup)
        sc = B * (S / 256.0) ** 2
        res = dict(workload=f"NAFNet-64 [1,1,1,28] fwd+L1+bwd+AdamW, B={B}, {S}x{S}, feature maps {args.dtype}",
                   ms_per_step=round(dt * 1e3, 2), megapixels_per_s=round(B * S * S / 1e6 / dt, 3), **rooflines(sc * 378.3e9, sc * naf_bytes, dt))
    elif args.workload == "dcpt":
        # configs[2]: NAFNet-64 encoder + PromptIR_NoImg_DC head, 10 classes, one DCPT step (fp32 here; the reference has no AMP)
        B, S = args.batch or 32, args.size or 128
        from basicsr.models import build_model

        opt = dict(name="b", model_type="DCPTModel", scale=1, num_gpu=1, dist=world > 1, rank=rank, world_size=world, is_train=True,
                   hook_names="decoder", network_g=dict(type="NAFNetBaseline", **naf),
                   network_dc=dict(type="PromptIR_NoImg_DC", feature_dims=[64, 128, 256, 512], num_res_blocks=2, num_classes=10,
                                   act_dtype=args.head_dtype or ("bf16" if bf else "fp32")),
                   path=dict(), train=dict(pixel_opt=dict(type="L1Loss"), classify_opt=dict(type="CrossEntropyLoss"),
                                           batched_encoder_passes=not args.two_pass,
                                           optim_g=dict(type="AdamW", lr=1e-4, fused=True), optim_dc=dict(type="AdamW", lr=1e-4, fused=True)))
        m = build_model(opt)   # (world > 1: both networks wrapped in DistributedDataParallel by BaseModel.model_to_device, reference base_model.py:108-115)
        fill_module_(m.get_bare_model(m.net_g))
        fill_module_(m.get_bare_model(m.net_dc))
        data = {"lq": torch.rand((B, 3, S, S), generator=g, device=dev), "gt": torch.rand((B, 3, S, S), generator=g, device=dev),
                "dataset_idx": torch.randint(0, 10, (B,), generator=g, device=dev)}
        m.feed_data(data)
        dt = timed(lambda: m.optimize_parameters(1), args.steps, args.warmup)
        sc = B * (S / 256.0) ** 2
        flops = sc * 1.315e12   # 1.315 TFLOP fwd+bwd per 256^2 image (2 x 378.3 GF encoder + 558.9 GF head)
        res = dict(workload=f"DCPT step: NAFNet-64 x2 fwd + PromptIR_NoImg_DC head + bwd (+ all-reduce of both networks' gradients) + 2x AdamW, "
                            f"B={B} per GPU, {S}x{S}, encoder feature maps {args.dtype}, head {args.head_dtype or args.dtype}",
                   ms_per_step=round(dt * 1e3, 2), megapixels_per_s=round(world * B * S * S / 1e6 / dt, 3), log=m.get_current_log())
        if bf:
            # two rooflines for the mixed step: the encoder's flops on the bf16 pipe + the head's on the fp32 pipe (time bound),
            # and the encoder's bf16 algorithmic bytes (the head's bytes are not in SURVEY 8d and are left out: a lower bound)
            head_peak = 2.5e15 if (args.head_dtype or "bf16") == "bf16" else 157.3e12
            t_mfma = sc * (2 * 378.3e9 / 2.5e15 + 558.9e9 / head_peak)
            t_hbm = sc * 2 * naf_bytes / 8e12
            res.update(alg_tflops=round(flops / dt / 1e12, 2), mfma_time_bound_ms=round(t_mfma * 1e3, 2), mfma_frac=round(t_mfma / dt, 4),
                       hbm_time_bound_ms_encoder_only=round(t_hbm * 1e3, 2), hbm_frac=round(t_hbm / dt, 4),
                       note="fractions = time bound / measured step; encoder bf16 (2.5 PF, bf16 bytes), head on its own pipe's peak")
        else:
            res.update(alg_tflops=round(flops / dt / 1e12, 2), mfma_frac=round(flops / dt / 157.3e12, 4))
    elif args.workload == "dcpt_swinir":
        # the SwinIR step of train_DCPT_SwinIR_5d.yml: 5D SwinIR encoder, token head on the three decoder RSTBs (hook_depth 0), fp32
        if args.dtype != "fp32" or world > 1:
            raise SystemExit("--workload dcpt_swinir: fp32, one GPU")
        B, S = args.batch or 8, args.size or 128
        from basicsr.models import build_model
        from dcpt_amd import functional as DF

        if args.torch_taps:   # bench-only: what the step would cost with the taps written as torch indexing
            dense_mix = DF.mix
            DF.tap_split = lambda x, lo, hi, stride=1: (x, x[lo:hi])
            DF.mix = lambda prev, feat, mw, idx, stride=1: dense_mix(prev, feat[:, :, ::stride, ::stride].contiguous(memory_format=torch.channels_last), mw, idx)
        opt = dict(name="b", model_type="DCPTModel", scale=1, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
                   hook_names="decode_layers", hook_depth=0,
                   network_g=dict(type="SwinIR", img_size=S, embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1),
                   network_dc=dict(type="PromptIR_NoImg_DC", feature_dims=[180, 180, 180], num_res_blocks=2, num_classes=5, downsample=True),
                   path=dict(), train=dict(pixel_opt=dict(type="L1Loss"), classify_opt=dict(type="CrossEntropyLoss"),
                                           batched_encoder_passes=not args.two_pass,
                                           optim_g=dict(type="AdamW", lr=1e-4, fused=True), optim_dc=dict(type="AdamW", lr=1e-4, fused=True)))
        m = build_model(opt)
        fill_module_(m.net_g)
        fill_module_(m.net_dc)
        m.feed_data({"lq": torch.rand((B, 3, S, S), generator=g, device=dev), "gt": torch.rand((B, 3, S, S), generator=g, device=dev),
                     "dataset_idx": torch.randint(0, 5, (B,), generator=g, device=dev)})
        dt = timed(lambda: m.optimize_parameters(1), args.steps, args.warmup)
        res = dict(workload=f"DCPT step: SwinIR 5D x2 fwd + PromptIR_NoImg_DC(downsample=True) head on decode_layers0..2 + bwd + 2x AdamW, B={B}, "
                            f"{S}x{S}, fp32, {'two passes' if args.two_pass else 'stacked pass'}, taps: "
                            f"{'torch indexing' if args.torch_taps else 'strided HIP kernels'}",
                   ms_per_step=round(dt * 1e3, 2), megapixels_per_s=round(B * S * S / 1e6 / dt, 3), log=m.get_current_log())
    elif args.workload == "restormer":
        if args.dtype not in ("fp32", "bf16"):
            raise SystemExit("--workload restormer: --dtype fp32 or bf16")
        res = run_restormer(dev, args.restormer_save, args.steps, args.warmup, args.batch or 64, args.size or 128, rank=rank, world=world,
                            dtype=args.dtype, grad_clip=args.grad_clip, ema_decay=args.ema_decay, fused_step_tail=args.fused_step_tail)
    elif args.workload == "promptir":
        if args.dtype not in ("fp32", "bf16"):
            raise SystemExit("--workload promptir: --dtype fp32 or bf16")
        res = run_promptir(dev, args.restormer_save, args.steps, args.warmup, args.batch or 32, args.size or 128, dtype=args.dtype)
    elif args.workload == "swinir":
        if (args.upsampler == "") != (args.upscale == 1):
            raise SystemExit("--upsampler and --upscale go together (an upsampler needs a scale above 1)")
        sr = args.upsampler != ""   # the SR forms are measured at 64 x 64 LR, training at the inference batch first
        if args.dtype not in ("fp32", "bf16", "bf16_res32") or (args.dtype != "fp32" and sr):
            raise SystemExit("--workload swinir: --dtype fp32, or bf16 / bf16_res32 for the restoration form's inference")
        res = run_swinir_bf16(dev, args.steps, args.warmup, args.batch or 8, args.size or 256, res32=args.dtype == "bf16_res32") if args.dtype != "fp32" else run_swinir(dev, args.steps, args.warmup, args.batch or 8, args.size or (64 if sr else 256),
                         train_batches=(args.batch or 8, 4, 2, 1) if sr else (12, 8, 4, 2, 1), upsampler=args.upsampler, upscale=args.upscale)
    elif args.workload == "rcan":
        if args.dtype not in ("fp32", "bf16", "bf16_res32"):
            raise SystemExit("--workload rcan: --dtype fp32, bf16 or bf16_res32")
        lines = run_rcan(dev, args.steps, args.warmup, args.batch or 16, args.size or 48, dtype=args.dtype)
        for line in lines[:-1]:
            print(json.dumps(line), flush=True)
        res = lines[-1]
    elif args.workload == "val_metrics":
        res = run_val_metrics(dev, args.steps, args.warmup)
    elif args.workload == "val_metrics_ms":
        lines = run_val_metrics_ms(dev, args.steps, args.warmup)
        for line in lines[:-1]:
            print(json.dumps(line), flush=True)
        res = lines[-1]
    elif args.workload == "step_tail":
        res = run_step_tail(dev, max(args.steps, 20), args.warmup)
    elif args.workload == "ssim_loss":
        res = run_ssim_loss(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 32, args.size or 256)
    elif args.workload == "ldl":
        res = run_ldl(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 32, args.size or 256)
    elif args.workload == "jpeg":
        res = run_jpeg(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 32, args.size or 256)
    elif args.workload == "niqe":
        res = run_niqe(dev, max(args.steps, 20), max(args.warmup, 3))
    elif args.workload == "degrade":
        lines = run_degrade(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 16, args.size or 256)
        print(json.dumps(lines[0]), flush=True)
        res = lines[1]
    elif args.workload == "noise":
        lines = run_noise(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 32, args.size or 256)
        print(json.dumps(lines[0]), flush=True)
        res = lines[1]
    elif args.workload == "blur":
        res = run_blur(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 32, args.size or 256)
    elif args.workload == "poisson":
        res = run_poisson(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 32, args.size or 256)
    elif args.workload == "degrade_chain":
        lines = run_degrade_chain(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 32, args.size or 256)
        print(json.dumps(lines[0]), flush=True)
        res = lines[1]
    elif args.workload == "knn":
        res = run_knn(dev, max(args.steps, 20), max(args.warmup, 3), args.batch or 500, args.size or 524288)
    elif args.workload == "tsne":
        lines = run_tsne(dev, (args.batch,) if args.batch else (500, 4096))
        for ln in lines[:-1]:
            print(json.dumps(ln), flush=True)
        res = lines[-1]
    elif args.workload == "tlsc":
        res = run_tlsc(dev, args.steps, args.warmup, tile=args.tile, streams=args.tile_streams)
    else:
        res = run_infer2k(dev, args.dtype, args.steps, args.warmup, args.size or 2048, args.tile_streams)
    res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    if world > 1:
        import torch.distributed as dist

        ones = torch.ones(1, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(ones)   # every rank that took part in the timed region contributes 1
        res.update(n_gpus=world, scaling="weak", parallelism=f"dp{world}", rccl_ranks=int(ones.item()) if dist.get_backend() == "nccl" else None)
        if args.path_check_shared_device:
            res["invalid"] = "path check: the ranks shared a device and the collectives went over gloo -- not a measurement"
        dist.barrier()
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
