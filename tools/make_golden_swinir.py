"""Golden vectors of the reference SwinIR (build container only; needs the reference tree).

    python tools/make_golden_swinir.py [REFERENCE_ROOT]

Imports the reference's basicsr/archs/swinir_arch.py under a private module name (its package __init__ is never executed) with a
three-name stand-in for ``timm.models.layers`` (to_2tuple, DropPath, trunc_normal_: only construction uses them, and with the
drop rates at 0 DropPath is never built), fills every state-dict entry with its keyed values (dcpt_amd.keyed_init) and writes
tests/golden/swinir_*.npz.  Single-threaded CPU float32, so a rerun reproduces the files bit for bit.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dcpt_amd.keyed_init import fill_module_, keyed_input, keyed_tensor  # noqa: E402
from oracle import ref_import  # noqa: E402  (REF: where the reference tree lives)

OUT = os.path.join(ROOT, "tests", "golden")
FULL = dict(embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
TINY = dict(embed_dim=36, depths=[2] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
# (tag, C, heads, window, shift, B, H, W): wrapped windows in both axes whenever shift > 0
BLOCKS = [("c180_s0", 180, 6, 8, 0, 1, 8, 24), ("c180_s4", 180, 6, 8, 4, 1, 8, 24),
          ("c60_ws4_s0", 60, 6, 4, 0, 2, 12, 16), ("c60_ws4_s2", 60, 6, 4, 2, 2, 12, 16)]
FULL_GRAD_MAX = 4096   # gradients up to this size are stored whole, larger ones as every 29th element (SUB)
SUB = 29


def load_reference_swinir(ref_root: str):
    def stub(name):
        m = types.ModuleType(name)
        m.__path__ = []
        return m

    saved = {k: v for k, v in sys.modules.items() if k == "basicsr" or k.startswith("basicsr.") or k == "timm" or k.startswith("timm.")}
    for k in saved:
        del sys.modules[k]
    try:
        timm, models, layers = stub("timm"), stub("timm.models"), stub("timm.models.layers")
        layers.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        layers.trunc_normal_ = lambda t, std=1.0, **kw: torch.nn.init.trunc_normal_(t, std=std)

        class DropPath(torch.nn.Module):
            def __init__(self, p=0.0):
                super().__init__()
                if p > 0:
                    raise RuntimeError("the golden configurations have no drop path")

            def forward(self, x):
                return x

        layers.DropPath = DropPath
        timm.models, models.layers = models, layers
        sys.modules.update({"timm": timm, "timm.models": models, "timm.models.layers": layers})
        for name, rel in [("basicsr", "basicsr"), ("basicsr.utils", "basicsr/utils"), ("basicsr.archs", "basicsr/archs")]:
            m = stub(name)
            m.__path__ = [os.path.join(ref_root, rel)]
            sys.modules[name] = m
        mods = {}
        for name, rel in [("basicsr.utils.registry", "basicsr/utils/registry.py"), ("basicsr.archs.swinir_arch", "basicsr/archs/swinir_arch.py")]:
            spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            mods[name] = mod
        return mods["basicsr.archs.swinir_arch"]
    finally:
        for k in [k for k in sys.modules if k == "basicsr" or k.startswith("basicsr.") or k == "timm" or k.startswith("timm.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32)


def _grads(module, out, keep_whole=lambda k: False, whole_max=FULL_GRAD_MAX):
    names, l2, s, a = [], [], [], []
    for k, p in module.named_parameters():
        g = p.grad.detach()
        names.append(k)
        gd = g.double()
        l2.append(float(gd.pow(2).sum().sqrt()))
        s.append(float(gd.sum()))
        a.append(float(gd.abs().sum()))
        if out is not None:
            if g.numel() <= whole_max or keep_whole(k):
                out["g." + k] = _np(g)
            else:
                out["gsub." + k] = _np(g.flatten()[::SUB])
    return np.array(names), np.array(l2), np.array(s), np.array(a)


def _tokens(x):   # (B, C, H, W) -> (B, L, C)
    return x.flatten(2).transpose(1, 2)


def _maps(t, H, W):   # (B, L, C) -> (B, C, H, W)
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], H, W)


def gen_blocks(S):
    for tag, C, heads, ws, shift, B, H, W in BLOCKS:
        blk = S.SwinTransformerBlock(dim=C, input_resolution=(128, 128), num_heads=heads, window_size=ws, shift_size=shift, mlp_ratio=2.0)
        blk.load_state_dict({k: keyed_tensor(f"swb_{tag}." + k, tuple(v.shape)) for k, v in blk.state_dict().items()}, strict=True)
        x = keyed_input(f"swb_{tag}.x", (B, C, H, W), lo=-1.0, hi=1.0).requires_grad_(True)
        go = keyed_input(f"swb_{tag}.go", (B, C, H, W), lo=-1.0, hi=1.0)
        y = _maps(blk(_tokens(x), (H, W)), H, W)
        y.backward(go)
        out = {"y": _np(y), "dx": _np(x.grad)}
        out["g_names"], out["g_l2"], out["g_sum"], out["g_abs"] = _grads(blk, out)
        np.savez_compressed(os.path.join(OUT, f"swinir_block_{tag}.npz"), **out)


def gen_tiny(S):
    net = S.SwinIR(**TINY)
    fill_module_(net, seed=0)
    x = keyed_input("swt.x", (2, 3, 32, 40)).requires_grad_(True)
    go = keyed_input("swt.go", (2, 3, 32, 40), lo=-1.0, hi=1.0)
    y = net(x)
    y.backward(go)
    out = {"y": _np(y), "dx": _np(x.grad)}
    whole = lambda k: k.startswith("encode_layers.0.residual_group.blocks.1.") or k.split(".")[0] in ("conv_first", "conv_last")   # noqa: E731
    out["g_names"], out["g_l2"], out["g_sum"], out["g_abs"] = _grads(net, out, whole, whole_max=512)
    np.savez_compressed(os.path.join(OUT, "swinir_tiny.npz"), **out)


def gen_full(S):
    net = S.SwinIR(**FULL)
    fill_module_(net, seed=0)
    sd = net.state_dict()
    x = keyed_input("swf.x", (1, 3, 64, 64)).requires_grad_(True)
    gt = keyed_input("swf.gt", (1, 3, 64, 64))
    y = net(x)
    loss = (y - gt).abs().mean()
    loss.backward()
    names, l2, s, a = _grads(net, None)
    out = {
        "y_sub": _np(y[..., ::4, ::4]),
        "y_mean": np.float64(y.double().mean().item()),
        "y_absmean": np.float64(y.double().abs().mean().item()),
        "loss": np.float64(loss.item()),
        "dx_sub": _np(x.grad[..., ::4, ::4]),
        "dx_l2": np.float64(x.grad.double().pow(2).sum().sqrt().item()),
        "g_names": names, "g_l2": l2, "g_sum": s, "g_abs": a,
        "keys": np.array(list(sd.keys())),
        "key_shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
        "n_params": np.int64(sum(p.numel() for p in net.parameters())),
        "n_keys": np.int64(len(sd)),
    }
    np.savez_compressed(os.path.join(OUT, "swinir_full.npz"), **out)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_import.REF
    torch.set_num_threads(1)
    torch.manual_seed(0)
    S = load_reference_swinir(ref_root)
    gen_blocks(S)
    gen_tiny(S)
    gen_full(S)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("swinir_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
