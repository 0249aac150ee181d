"""Golden vectors of the reference SwinIR in its three super-resolution forms and with the 3conv residual (build container only;
needs the reference tree).

    python tools/make_golden_swinir_sr.py [REFERENCE_ROOT]

Loads the reference's swinir_arch.py exactly as tools/make_golden_swinir.py does, fills every state-dict entry with its keyed values
(dcpt_amd.keyed_init) and writes tests/golden/swinir_sr_*.npz: arrays and key names only.  Single-threaded CPU float32, so a rerun
reproduces the files bit for bit.

  swinir_sr_<form>_x<r>.npz   tiny nets (the TINY body of make_golden_swinir.py, embed 36): y, dx and the parameter gradients (small ones
                              whole, larger ones as every 29th element) for pixelshuffle x2 / x3 / x4, pixelshuffledirect x2 / x3 / x4,
                              nearest+conv x2 / x4; swinir_sr_nearestconv_x4_3conv.npz the same with resi_connection="3conv" at embed 48
  swinir_sr_key_*.npz         state-dict keys, shapes, parameter count and a sub-sampled forward output of classical x4 at width 180,
                              lightweight x2 at width 60 and 3conv real-world x4 at width 240
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dcpt_amd.keyed_init import fill_module_, keyed_input  # noqa: E402
from oracle import ref_import  # noqa: E402  (REF: where the reference tree lives)
from make_golden_swinir import OUT, TINY, _grads, _np, load_reference_swinir  # noqa: E402

TAGS = {"pixelshuffle": "pixelshuffle", "pixelshuffledirect": "direct", "nearest+conv": "nearestconv"}
# (upsampler, upscale, resi_connection, embed_dim, (H, W))
TINY_NETS = [("pixelshuffle", 2, "1conv", 36, (16, 24)), ("pixelshuffle", 3, "1conv", 36, (16, 16)), ("pixelshuffle", 4, "1conv", 36, (16, 16)),
             ("pixelshuffledirect", 2, "1conv", 36, (16, 24)), ("pixelshuffledirect", 3, "1conv", 36, (16, 16)),
             ("pixelshuffledirect", 4, "1conv", 36, (16, 16)),
             ("nearest+conv", 2, "1conv", 36, (16, 24)), ("nearest+conv", 4, "1conv", 36, (16, 16)),
             ("nearest+conv", 4, "3conv", 48, (16, 16))]
# (tag, constructor arguments): the published classical, lightweight and real-world (3conv, "large") configurations
KEY_NETS = [("classical_x4_c180", dict(embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, upsampler="pixelshuffle", upscale=4)),
            ("lightweight_x2_c60", dict(embed_dim=60, depths=[6] * 6, num_heads=[6] * 6, upsampler="pixelshuffledirect", upscale=2)),
            ("realworld_x4_c240_3conv", dict(embed_dim=240, depths=[6] * 6, num_heads=[8] * 6, upsampler="nearest+conv", upscale=4,
                                             resi_connection="3conv"))]


def tiny_name(upsampler, r, resi):
    return f"swinir_sr_{TAGS[upsampler]}_x{r}" + ("_3conv" if resi == "3conv" else "") + ".npz"


def tiny_kwargs(upsampler, r, resi, embed):
    return dict(TINY, embed_dim=embed, upscale=r, upsampler=upsampler, resi_connection=resi, img_size=64)


def gen_tiny(S):
    for upsampler, r, resi, embed, (H, W) in TINY_NETS:
        net = S.SwinIR(**tiny_kwargs(upsampler, r, resi, embed))
        fill_module_(net, seed=0)
        tag = tiny_name(upsampler, r, resi)[:-4]
        x = keyed_input(tag + ".x", (2, 3, H, W)).requires_grad_(True)
        go = keyed_input(tag + ".go", (2, 3, r * H, r * W), lo=-1.0, hi=1.0)
        y = net(x)
        y.backward(go)
        out = {"y": _np(y), "dx": _np(x.grad)}
        body = ("encode_layers", "decode_layers0", "decode_layers1", "decode_layers2")
        whole = lambda k: k.split(".")[0] not in body and p_small[k]   # noqa: E731
        p_small = {k: p.numel() <= 8192 for k, p in net.named_parameters()}
        out["g_names"], out["g_l2"], out["g_sum"], out["g_abs"] = _grads(net, out, whole, whole_max=512)
        np.savez_compressed(os.path.join(OUT, tiny_name(upsampler, r, resi)), **out)


def gen_keys(S):
    for tag, kw in KEY_NETS:
        net = S.SwinIR(img_size=64, window_size=8, mlp_ratio=2.0, **kw)
        fill_module_(net, seed=0)
        sd = net.state_dict()
        with torch.no_grad():
            y = net(keyed_input(f"swinir_sr_key_{tag}.x", (1, 3, 16, 16)))
        out = {
            "y_sub": _np(y[..., ::2, ::2]),
            "y_absmean": np.float64(y.double().abs().mean().item()),
            "keys": np.array(list(sd.keys())),
            "key_shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
            "n_params": np.int64(sum(p.numel() for p in net.parameters())),
        }
        np.savez_compressed(os.path.join(OUT, f"swinir_sr_key_{tag}.npz"), **out)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_import.REF
    torch.set_num_threads(1)
    torch.manual_seed(0)
    S = load_reference_swinir(ref_root)
    gen_tiny(S)
    gen_keys(S)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("swinir_sr_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
