#!/usr/bin/env python
"""The equality probe for changes that must not change what the ops compute: for every op of dcpt_amd/functional.py in the list below,
on seeded inputs (dcpt_amd.keyed_init), one forward + backward and into ONE JSON file

  * the SHA-256 of every output and gradient tensor (its bytes as stored, fp32 or bf16),
  * the text of the library's launch trace for the run (dcpt_trace_read: which kernel family ran how often),
  * under tests/redzone.py ``redzone(fill=False)``, the sizes requested from the three allocators, in order.

Run it in two trees (one process each, same box) and compare the files byte for byte:

    python tools/op_bits.py --out bits_parent.json     # in the parent's tree
    python tools/op_bits.py --out bits_head.json       # in the head's tree
    cmp bits_parent.json bits_head.json

The file holds nothing that differs between two runs of one tree (no paths, times or addresses)."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from dcpt_amd import _lib  # noqa: E402
from dcpt_amd import functional as DF  # noqa: E402
from dcpt_amd.keyed_init import keyed_input, keyed_tensor  # noqa: E402
from redzone import redzone  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16


class Case:
    """one op call: ``leaves`` collects every tensor whose gradient is recorded; ``after`` undoes a setting the case changed"""

    def __init__(self, name):
        self.name, self.leaves, self.after = name, {}, None

    def fmap(self, tag, b, c, h, w, bf=False, grad=True):
        x = keyed_input(f"{self.name}.{tag}", (b, c, h, w), lo=-1.0, hi=1.0).to(DEV).contiguous(memory_format=torch.channels_last)
        x = (x.to(BF) if bf else x).requires_grad_(grad)
        if grad:
            self.leaves[tag] = x
        return x

    def image(self, tag, b, c, h, w, grad=False):
        x = keyed_input(f"{self.name}.{tag}", (b, c, h, w)).to(DEV).requires_grad_(grad)
        if grad:
            self.leaves[tag] = x
        return x

    def par(self, tag, *shape, offset=0.0, grad=True):
        p = (keyed_tensor(f"{self.name}.{tag}", shape) + offset).to(DEV).requires_grad_(grad)
        if grad:
            self.leaves[tag] = p
        return p

    def conv(self, tag, cout, cin, k, grad=True):
        return self.par(tag + ".weight", cout, cin, k, k, grad=grad), self.par(tag + ".bias", cout, grad=grad)

    def ln(self, tag, c):
        return self.par(tag + ".w", c, offset=1.0), self.par(tag + ".b", c)


def _nafblock_params(k, c, grad=True):
    shapes = dict(norm1_w=(c,), norm1_b=(c,), conv1_w=(2 * c, c, 1, 1), conv1_b=(2 * c,), conv2_w=(2 * c, 1, 3, 3), conv2_b=(2 * c,),
                  conv3_w=(c, c, 1, 1), conv3_b=(c,), sca_w=(c, c, 1, 1), sca_b=(c,), norm2_w=(c,), norm2_b=(c,), conv4_w=(2 * c, c, 1, 1),
                  conv4_b=(2 * c,), conv5_w=(c, c, 1, 1), conv5_b=(c,), beta=(1, c, 1, 1), gamma=(1, c, 1, 1))
    return {n: k.par(n, *shapes[n], offset=1.0 if n in ("norm1_w", "norm2_w") else 0.0, grad=grad) for n in _lib.PARAM_FIELDS}


def _nafblock_bf16(k, c, hw, packed):
    """bf16 storage at another width: ``packed`` = through a PackedWeightsBf16 cache, else packed in the call"""
    return DF.nafblock_bf16(k.fmap("x", 2, c, hw, hw, True), _nafblock_params(k, c), packed=DF.PackedWeightsBf16() if packed else None)


def _nafblock_local_bf16(k, c, hw, packed):
    return DF.nafblock_local_bf16(k.fmap("x", 2, c, hw, hw, True, grad=False), _nafblock_params(k, c, grad=False), 5, 7,
                                  packed=DF.PackedWeightsBf16() if packed else None)


def _bottleneck(k, bf, b, c, cb, h, w, packed=False):
    """cb = 2 c: the geometry of the one-call bf16 entry points; any other mid width: one call per conv -> LayerNorm group"""
    ps = (k.par("conv1", cb, c, 1, 1), *k.ln("ln1", cb), k.par("conv2", cb, cb, 3, 3), *k.ln("ln2", cb), k.par("conv3", c, cb, 1, 1), *k.ln("ln3", c))
    return DF.bottleneck(k.fmap("x", b, c, h, w, bf), *ps, packs=tuple(DF.PackedConvBf16() for _ in range(3)) if packed else None)


def _wgrad_bf16(k, m, n, kk, with_bias):
    dy = keyed_input(f"{k.name}.dy", (m, n), lo=-1.0, hi=1.0).to(DEV).to(BF)
    x = keyed_input(f"{k.name}.x", (m, kk), lo=-1.0, hi=1.0).to(DEV).to(BF)
    return DF.conv1x1_wgrad_bf16(dy, x, with_bias=with_bias)


def _nafblock(k, bf, c=64, hw=16):
    params = _nafblock_params(k, c)
    x = k.fmap("x", 2, c, hw, hw, bf)
    return DF.nafblock_bf16(x, params) if bf else DF.nafblock(x, params)


def _mdta(k, bf, biasfree):
    c, heads = 48, 2
    nw, nb = k.ln("norm", c)
    return DF.mdta(k.fmap("x", 2, c, 13, 17 if not bf else 16, bf), nw, None if biasfree else nb, k.par("qkv", 3 * c, c, 1, 1),
                   k.par("dw", 3 * c, 1, 3, 3), k.par("proj", c, c, 1, 1), k.par("temp", heads, 1, 1, offset=1.0), heads, biasfree)


def _gdfn(k, bf, biasfree):
    c, hid = 48, 127
    nw, nb = k.ln("norm", c)
    return DF.gdfn(k.fmap("x", 2, c, 13, 17 if not bf else 16, bf), nw, None if biasfree else nb, k.par("in", 2 * hid, c, 1, 1),
                   k.par("dw", 2 * hid, 1, 3, 3), k.par("out", c, hid, 1, 1), biasfree)


def _swin_attn(k, shift):
    c, heads = 60, 6
    return DF.swin_attn(k.fmap("x", 2, c, 16, 16), *k.ln("norm", c), k.par("qkv_w", 3 * c, c), k.par("qkv_b", 3 * c), k.par("proj_w", c, c),
                        k.par("proj_b", c), heads, 8, shift)


def _swin_mlp(k):
    c = 60
    return DF.swin_mlp(k.fmap("x", 2, c, 16, 16), *k.ln("norm", c), k.par("fc1_w", 2 * c, c), k.par("fc1_b", 2 * c), k.par("fc2_w", c, 2 * c),
                       k.par("fc2_b", c))


def _rcab_params(k, c, cr, grad=True):
    return (*k.conv("c1", c, c, 3, grad), *k.conv("c2", c, c, 3, grad), *k.conv("ca1", cr, c, 1, grad), *k.conv("ca2", c, cr, 1, grad))


def _conv_ln(k, bf, ks):
    x, res = k.fmap("x", 2, 64, 13, 16 if bf else 17, bf), k.fmap("res", 2, 128, 13, 16 if bf else 17, bf)
    return (DF.conv_ln_bf16 if bf else DF.conv_ln)(x, k.par("weight", 128, 64, ks, ks), *k.ln("ln", 128), res, True)


def _conv3conv_res(k):
    c, q = 48, 12
    return DF.conv3conv_res(k.fmap("x", 2, c, 13, 17), *k.conv("1", q, c, 3), *k.conv("2", q, q, 1), *k.conv("3", c, q, 3), k.fmap("res", 2, c, 13, 17))


def _ssim_pt(k, luma):
    """three images through the backward's chunk loop one at a time: the plane cap holds one image's Pa, Pb, Pc"""
    b, c, h, w, crop = 3, 3, 29, 45, 1
    cap = DF.ssim_plane_cap()
    k.after = lambda: DF.ssim_plane_cap(cap)   # (the chunk loop is the backward's: the cap stays until _run is through)
    DF.ssim_plane_cap((1 if luma else c) * 3 * (h - 2 * crop - 10) * (w - 2 * crop - 10) * 8)
    return DF.ssim_pt(k.image("pred", b, c, h, w, grad=True), k.image("target", b, c, h, w), crop, luma)


def _tsne(k):
    """affinities, three descent steps and the KL divergence at N = 300 (more than one stride of the 256 lanes)"""
    n = 300
    x = keyed_input(f"{k.name}.x", (n, 8), lo=-1.0, hi=1.0).double()
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    d2 = (0.5 * (d2 + d2.t())).to(DEV)
    y = (keyed_input(f"{k.name}.y", (n, 2), lo=-1.0, hi=1.0).double() * 1e-2).to(DEV)
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    p, beta, steps = DF.tsne_affinities(d2, 30.0)
    stats = DF.tsne_steps(p, y, update, gains, 3, 12.0, 0.5, 200.0)
    kl, grad = DF.tsne_kl(p, y)
    return p, beta, steps, y, update, gains, stats, kl.reshape(1), grad


def _cases():
    """(name, f(Case) -> output or tuple of outputs, needs backward)"""
    out = []

    def add(name, fn, backward=True):
        out.append((name, fn, backward))

    # the list of LABNOTES 4p ("MI355X, bits")
    for shift in (0, 4):
        add(f"swin_attn.shift{shift}", lambda k, s=shift: _swin_attn(k, s))
    add("swin_mlp", _swin_mlp)
    add("conv3x3_res", lambda k: DF.conv3x3_res(k.fmap("x", 2, 60, 13, 17), *k.conv("conv", 60, 60, 3), k.fmap("res", 2, 60, 13, 17)))
    add("rcab", lambda k: DF.rcab(k.fmap("x", 2, 64, 13, 17), *_rcab_params(k, 64, 4), res_scale=0.5))
    for r in (2, 3):
        add(f"conv3x3_ps.r{r}", lambda k, r=r: DF.conv3x3_ps(k.fmap("x", 2, 64, 13, 17), *k.conv("conv", r * r * 64, 64, 3), r))
    add("conv3x3_act", lambda k: DF.conv3x3_act(k.fmap("x", 2, 60, 13, 17), *k.conv("conv", 64, 60, 3), 0.2))
    add("up2_conv3x3_act", lambda k: DF.up2_conv3x3_act(k.fmap("x", 2, 64, 13, 17), *k.conv("conv", 64, 64, 3), 0.2))
    add("conv3x3_ps_out", lambda k: DF.conv3x3_ps_out(k.fmap("x", 2, 60, 13, 17), *k.conv("conv", 27, 60, 3), 3))
    add("conv3conv_res", _conv3conv_res)
    for ks in (1, 3):
        add(f"conv_ln.k{ks}", lambda k, ks=ks: _conv_ln(k, False, ks))
    add("nafblock", lambda k: _nafblock(k, False))
    for bfree in (False, True):
        tag = "biasfree" if bfree else "withbias"
        add(f"mdta.{tag}", lambda k, b=bfree: _mdta(k, False, b))
        add(f"gdfn.{tag}", lambda k, b=bfree: _gdfn(k, False, b))
    # their bf16-storage forms
    add("nafblock_bf16", lambda k: _nafblock(k, True))
    for ks in (1, 3):
        add(f"conv_ln_bf16.k{ks}", lambda k, ks=ks: _conv_ln(k, True, ks))
    for bfree in (False, True):
        tag = "biasfree" if bfree else "withbias"
        add(f"mdta_bf16.{tag}", lambda k, b=bfree: _mdta(k, True, b))
        add(f"gdfn_bf16.{tag}", lambda k, b=bfree: _gdfn(k, True, b))
    add("rcab_bf16", lambda k: DF.rcab_bf16(k.fmap("x", 2, 64, 13, 16, True, grad=False), *_rcab_params(k, 64, 4, grad=False), res_scale=0.5), False)
    add("conv3x3_res_bf16", lambda k: DF.conv3x3_res_bf16(k.fmap("x", 2, 64, 13, 16, True, grad=False), *k.conv("conv", 64, 64, 3, grad=False),
                                                            k.fmap("res", 2, 64, 13, 16, True, grad=False)), False)
    for r in (2, 3):
        add(f"conv3x3_ps_bf16.r{r}", lambda k, r=r: DF.conv3x3_ps_bf16(k.fmap("x", 2, 64, 13, 16, True, grad=False),
                                                                      *k.conv("conv", r * r * 64, 64, 3, grad=False), r), False)
    # the NAFNet / head / Restormer glue ops, both storages
    add("layernorm2d", lambda k: DF.layernorm2d(k.fmap("x", 2, 64, 13, 17), *k.ln("ln", 64)))
    for bf in (False, True):
        s = "_bf16" if bf else ""
        add("conv3x3_in" + s, lambda k, bf=bf: DF.conv3x3_in(k.image("x", 2, 3, 14, 16), *k.conv("conv", 64, 3, 3), out_bf16=bf))
        add("conv3x3_out" + s, lambda k, bf=bf: DF.conv3x3_out(k.fmap("x", 2, 64, 14, 16, bf), *k.conv("conv", 3, 64, 3), k.image("res", 2, 3, 14, 16)))
        add("down2x2" + s, lambda k, bf=bf: DF.down2x2(k.fmap("x", 2, 64, 14, 16, bf), *k.conv("conv", 128, 64, 2)))
        add("down2x2_skip" + s, lambda k, bf=bf: DF.down2x2_skip(k.fmap("x", 2, 64, 14, 16, bf), *k.conv("conv", 128, 64, 2)))
        add("up_ps" + s, lambda k, bf=bf: DF.up_ps(k.fmap("x", 2, 64, 7, 8, bf), k.par("weight", 128, 64, 1, 1), k.fmap("skip", 2, 32, 14, 16, bf)))
        add("conv_nobias" + s, lambda k, bf=bf: DF.conv_nobias(k.fmap("x", 2, 48, 13, 16, bf), k.par("weight", 96, 48, 3, 3)))
        add("pixel_shuffle2" + s, lambda k, bf=bf: DF.pixel_shuffle2(k.fmap("x", 2, 64, 13, 16, bf)))
        add("concat_channels" + s, lambda k, bf=bf: DF.concat_channels(k.fmap("a", 2, 48, 13, 16, bf), k.fmap("b", 2, 24, 13, 16, bf)))
        add("conv1x1_pool_relu" + s, lambda k, bf=bf: (DF.conv1x1_pool_relu_bf16 if bf else DF.conv1x1_pool_relu)(
            k.fmap("x", 2, 64, 14, 16, bf), k.par("weight", 128, 64, 1, 1)))
        add("mix" + s, lambda k, bf=bf: DF.mix(k.fmap("prev", 2, 64, 14, 16, bf), k.fmap("feat", 2, 64, 14, 16, bf), k.par("w", 4), 1))
        add("prompt_mix" + s, lambda k, bf=bf: DF.prompt_mix(k.par("logits", 2, 5), k.par("param", 1, 5, 64, 16, 16), 14, 16, out_bf16=bf))
    # the bf16 op host layer (LABNOTES 4r): the paths of the 128-tile weight-gradient helper, the 256-tile launch + finisher, the cached
    # operand images and the TLSC forward that the cases above do not reach
    add("bottleneck_bf16.c16.one_call", lambda k: _bottleneck(k, True, 2, 16, 32, 6, 10))
    add("bottleneck_bf16.c16.one_call.packed", lambda k: _bottleneck(k, True, 2, 16, 32, 6, 10, packed=True))
    add("bottleneck_bf16.c16.per_group", lambda k: _bottleneck(k, True, 2, 16, 24, 6, 10))
    add("bottleneck_bf16.c128", lambda k: _bottleneck(k, True, 1, 128, 256, 16, 16))   # conv2's weight gradient: 256-tile kernel + finisher
    for m, n, kk in ((300, 256, 512), (513, 64, 128)):
        for wb in (True, False):
            add(f"conv1x1_wgrad_bf16.{m}x{n}x{kk}.{'bias' if wb else 'nobias'}", lambda k, a=(m, n, kk), wb=wb: _wgrad_bf16(k, *a, wb), False)
    for pk in (True, False):
        add(f"nafblock_bf16.c256.{'packed' if pk else 'unpacked'}", lambda k, pk=pk: _nafblock_bf16(k, 256, 16, pk))   # grouped launch + finisher
        add(f"nafblock_bf16.c128.{'packed' if pk else 'unpacked'}", lambda k, pk=pk: _nafblock_bf16(k, 128, 8, pk))    # four 128-tile weight gradients
        add(f"nafblock_local_bf16.c64.{'packed' if pk else 'unpacked'}", lambda k, pk=pk: _nafblock_local_bf16(k, 64, 16, pk), False)
    add("conv_nobias_bf16.k1", lambda k: DF.conv_nobias(k.fmap("x", 2, 48, 13, 16, True), k.par("weight", 96, 48, 1, 1)))
    # the fp64 window, block-sum and reduce kernels (metrics, MS-SSIM, MATLAB SSIM, range, SSIM loss, LDL, t-SNE) at the smallest shapes that
    # reach every ragged edge of the 16 x 32 tile under the window of 11: (29, 45) cropped by 1 leaves a 17 x 33 map, 2 x 2 tiles whose last
    # row and column hold one position
    pair = lambda k, *s: (k.image("a", *s), k.image("b", *s))   # noqa: E731
    for rng in (255, 1):
        for luma in (False, True):
            tag = f"r{rng}.{'y' if luma else 'rgb'}"
            add(f"image_metric_sums.{tag}", lambda k, r=rng, y=luma: DF.image_metric_sums(*pair(k, 2, 3, 29, 45), 1, y, r), False)
    add("image_metric_sums.psnr_only", lambda k: DF.image_metric_sums(*pair(k, 1, 3, 5, 7), ssim=False)[0], False)
    add("msssim_sums.l5.rgb", lambda k: DF.msssim_sums(*pair(k, 2, 3, 29, 45), 1, False, 255, 5), False)   # the channel cycles k mod 3
    add("msssim_sums.l8.y.r1", lambda k: DF.msssim_sums(*pair(k, 2, 3, 29, 45), 1, True, 1, 8), False)
    add("ssim_matlab_sums", lambda k: DF.ssim_matlab_sums(*pair(k, 2, 3, 17, 33), 0), False)
    add("ssim_matlab_sums.narrow", lambda k: DF.ssim_matlab_sums(*pair(k, 1, 1, 5, 7), 1), False)   # narrower than the halo: clamps on both sides
    add("image_range_minmax", lambda k: DF.image_range_minmax(k.image("a", 2, 3, 40, 61), 1), False)   # 6726 values: two chunks, the second ragged
    for luma in (False, True):
        add(f"ssim_pt.{'y' if luma else 'rgb'}", lambda k, y=luma: _ssim_pt(k, y))
    add("ldl_weight", lambda k: DF.ldl_weight(k.image("gt", 2, 3, 17, 33), k.image("out", 2, 3, 17, 33, grad=True)))
    add("ldl_weight.5x5", lambda k: DF.ldl_weight(k.image("gt", 1, 1, 5, 5), k.image("out", 1, 1, 5, 5, grad=True)))   # both reflect folds on the same pixels
    add("tsne", _tsne, False)
    return out


def _sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _trace_text(lib):
    need = lib.dcpt_trace_read(None, 0)
    buf = ctypes.create_string_buffer(int(need) + 16)
    lib.dcpt_trace_read(buf, len(buf))
    return buf.value.decode()


def _run(name, fn, backward):
    """-> ({tensor name: sha256}, outputs kept alive)"""
    k = Case(name)
    try:
        if backward:
            res = fn(k)
        else:
            with torch.no_grad():
                res = fn(k)
        outs = list(res) if isinstance(res, tuple) else [res]
        hashes = {}
        if backward:
            loss = 0
            for i, o in enumerate(outs):
                cot = keyed_input(f"{name}.cot{i}", tuple(o.shape), lo=-1.0, hi=1.0).to(DEV)
                loss = loss + (o.float() * cot).sum()
            loss.backward()
            for tag, leaf in k.leaves.items():
                if leaf.grad is not None:
                    hashes["grad." + tag] = _sha(leaf.grad)
        for i, o in enumerate(outs):
            hashes[f"out{i}"] = _sha(o)
        torch.cuda.synchronize()
    finally:
        if k.after:
            k.after()
    return hashes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="", help="substring of the case names to run")
    args = ap.parse_args()
    lib = _lib.load()
    result = {}
    for name, fn, backward in _cases():
        if args.only not in name:
            continue
        lib.dcpt_trace_enable(1)
        try:
            hashes = _run(name, fn, backward)
            trace = _trace_text(lib)
        finally:
            lib.dcpt_trace_enable(0)
        with redzone(fill=False) as rz:
            _run(name, fn, backward)
            sizes = [n for _, _, n in rz.allocs]
        result[name] = {"sha256": hashes, "trace": trace.splitlines(), "alloc_bytes": sizes}
        print(f"{name}: {len(hashes)} tensors, {len(sizes)} allocations", flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(result)} cases, {sum(len(v['sha256']) for v in result.values())} tensors")


if __name__ == "__main__":
    main()
