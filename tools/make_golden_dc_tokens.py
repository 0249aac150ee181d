"""Golden vectors of the reference's token-tap classifier head and of its SwinIR DCPT step (build container only; needs the
reference tree).

    python tools/make_golden_dc_tokens.py

``PromptIR_NoImg_DC(downsample=True)`` (reference basicsr/archs/degrad_classify_arch.py:558-641) is imported through
oracle.ref_import, the reference SwinIR through tools/make_golden_swinir.py's loader; every state-dict entry gets its keyed values
(dcpt_amd.keyed_init).  Single-threaded CPU float32, so a rerun reproduces the files bit for bit.

tests/golden/dc_head_tokens.npz   the head alone on (B, L, C) token features: logits, loss, the gradient of every feature, of
                                  mixing_weights and of a fixed parameter sample, the L2 norm of every parameter gradient
tests/golden/dcpt_step_swinir.npz one DCPT step composed as ...pretrain_model.py:133-169: net_g(gt) -> L1; net_g(lq) with forward hooks
                                  on decode_layers0..2; head on the taps reversed -> CE; one backward
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dcpt_amd.keyed_init import fill_module_, keyed_input  # noqa: E402
from oracle import ref_import  # noqa: E402
from make_golden_swinir import FULL_GRAD_MAX, SUB, TINY, load_reference_swinir  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NUM_CLASSES = 5
# (tag, feature_dims, num_res_blocks): equal widths as SwinIR's taps have, and unequal ones so that every downsample conv changes width
HEAD_CASES = [("a", [12, 12, 12], 1), ("b", [8, 16, 12], 2)]
HEAD_SAMPLE = ["mixing_weights", "fc.weight", "fc.bias", "bottleneck_layers.0.0.conv1.weight", "bottleneck_layers.1.0.conv2.norm.weight",
               "downsample_layers.1.0.weight", "last_stage.0.conv3.weight"]
HEAD_LABELS = [3, 1]
STEP_IMG = 16
STEP_HEAD = dict(feature_dims=[36, 36, 36], num_res_blocks=1, num_classes=NUM_CLASSES, downsample=True)
STEP_LABELS = [4, 2]


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32)


def _l2(module):
    names = [k for k, _ in module.named_parameters()]
    return np.array(names), np.array([float(p.grad.double().pow(2).sum().sqrt()) for _, p in module.named_parameters()])


def gen_head(dc):
    out = {}
    for tag, dims, nrb in HEAD_CASES:
        net = dc.PromptIR_NoImg_DC(feature_dims=list(dims), num_res_blocks=nrb, num_classes=NUM_CLASSES, downsample=True)
        fill_module_(net, seed=0)
        feats = [keyed_input(f"dct.{tag}.f{i}", (2, 256, c), lo=-1.0, hi=1.0).requires_grad_(True) for i, c in enumerate(dims)]
        logits = net(None, list(feats))   # (the reference overwrites the entries of the list it is given)
        loss = F.cross_entropy(logits, torch.tensor(HEAD_LABELS))
        loss.backward()
        out[f"{tag}.logits"], out[f"{tag}.loss"] = _np(logits), np.float64(loss.item())
        for i, f in enumerate(feats):
            out[f"{tag}.df{i}"] = _np(f.grad)
        params = dict(net.named_parameters())
        for k in HEAD_SAMPLE:
            out[f"{tag}.g.{k}"] = _np(params[k].grad)
        out[f"{tag}.g_names"], out[f"{tag}.g_l2"] = _l2(net)
        out[f"{tag}.keys"] = np.array(list(net.state_dict().keys()))
    out["cases"] = np.array([t for t, _, _ in HEAD_CASES])
    np.savez_compressed(os.path.join(OUT, "dc_head_tokens.npz"), **out)


def gen_step(S, dc):
    net_g = S.SwinIR(img_size=STEP_IMG, **TINY)
    net_dc = dc.PromptIR_NoImg_DC(**STEP_HEAD)
    fill_module_(net_g, seed=0)
    fill_module_(net_dc, seed=0)
    gt = keyed_input("dcsw.gt", (2, 3, STEP_IMG, STEP_IMG))
    lq = keyed_input("dcsw.lq", (2, 3, STEP_IMG, STEP_IMG))
    taps = []
    hooked = [f"decode_layers{i}" for i in range(3)]
    for name in hooked:   # what the one-dot rule of :65-68 selects on the DDP-wrapped net: the decoder RSTBs themselves
        getattr(net_g, name).register_forward_hook(lambda m, i, o: taps.append(o[-1] if isinstance(o, tuple) else o))
    pix = net_g(gt, hook=False)
    taps.clear()
    l_pix = F.l1_loss(pix, gt)
    net_g(lq, hook=True)
    assert len(taps) == 3 and all(t.dim() == 3 for t in taps)
    logits = net_dc(lq, taps[::-1])
    l_cls = F.cross_entropy(logits, torch.tensor(STEP_LABELS))
    (l_pix + l_cls).backward()
    out = {"l_pix": np.float64(l_pix.item()), "l_classify": np.float64(l_cls.item()), "logits": _np(logits), "hooked": np.array(hooked),
           "tap_shape": np.array(taps[0].shape)}
    for tag, net in (("g", net_g), ("dc", net_dc)):
        out[f"{tag}_names"], out[f"{tag}_l2"] = _l2(net)
        for k, p in net.named_parameters():
            g = p.grad.detach()
            if g.numel() <= FULL_GRAD_MAX:
                out[f"{tag}.g.{k}"] = _np(g)
            else:
                out[f"{tag}.gsub.{k}"] = _np(g.flatten()[::SUB])
    np.savez_compressed(os.path.join(OUT, "dcpt_step_swinir.npz"), **out)


def main():
    torch.set_num_threads(1)
    torch.manual_seed(0)
    warnings.filterwarnings("ignore", category=UserWarning)   # (the reference calls softmax without a dim)
    dc = ref_import.load_reference_archs().dc
    if dc is None:
        raise RuntimeError("the reference's degrad_classify_arch did not import")
    S = load_reference_swinir(ref_import.REF)
    gen_head(dc)
    gen_step(S, dc)
    for f in ("dc_head_tokens.npz", "dcpt_step_swinir.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
