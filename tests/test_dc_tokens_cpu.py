"""CPU: the token-tap classifier head (PromptIR_NoImg_DC(downsample=True)) and the SwinIR DCPT step around it -- the strided-tap entry
points in header / ctypes table / library, hook selection (hook_depth), the head's input validation, the golden files."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dcpt_grid_add", "dcpt_grid_scatter", "dcpt_mix_stride_bwd", "dcpt_mix_stride_bwd_ws_bytes", "dcpt_mix_stride_fwd"]
NETS = {
    "naf": (dict(type="NAFNetBaseline", img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 2], dec_blk_nums=[1, 1, 1, 1]),
            "decoder", ["decoder0.0", "decoder1.0", "decoder2.0", "decoder3.0"]),
    "restormer": (dict(type="Restormer", dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, heads=[1, 2, 4, 8]),
                  "decoder_level", ["decoder_level3.body", "decoder_level2.body", "decoder_level1.body"]),
    "promptir": (dict(type="PromptIR", num_blocks=[1, 1, 1, 1], num_refinement_blocks=1),
                 "decoder_level", ["decoder_level3.0", "decoder_level2.0", "decoder_level1.0"]),
}
SWIN_TINY = dict(type="SwinIR", img_size=16, embed_dim=36, depths=[2] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)


def test_new_entry_points_in_header_table_and_library():
    from dcpt_amd import _lib, build

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcpt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dcpt_[a-z0-9_]+)\s*\(", txt))
    exported = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/dcpt_hip.h"
        assert s in _lib.SIGNATURES, f"{s} is not in dcpt_amd._lib.SIGNATURES"
        assert s in exported, f"{s} is not exported by the library"
    lib = _lib.load()
    assert lib.dcpt_abi_version() == _lib.ABI_VERSION == 16
    assert lib.dcpt_mix_stride_bwd_ws_bytes(2 * 4 * 4 * 180) == lib.dcpt_mix_bwd_ws_bytes(2 * 4 * 4 * 180) > 0


def test_bad_strided_arguments_are_reported_before_any_launch():
    from dcpt_amd import _lib

    lib = _lib.load()
    p = 4096   # (never dereferenced: every call below fails its argument check)
    bad = [dict(C=6), dict(s=3), dict(H=12, s=8), dict(W=4, s=8), dict(s=0), dict(sw=6), dict(sh=130)]
    for over in bad:
        a = dict(B=2, H=8, W=8, C=8, s=2, sb=512, sh=64, sw=8)
        a.update(over)
        rc = lib.dcpt_mix_stride_fwd(None, p, p, 3, 1, p, a["B"], a["H"], a["W"], a["C"], a["s"], a["sb"], a["sh"], a["sw"], None)
        assert rc == 1 and b"mix_stride_fwd" in lib.dcpt_last_error(), over
    assert lib.dcpt_mix_stride_fwd(None, p, p, 3, 3, p, 2, 8, 8, 8, 2, 512, 64, 8, None) == 1    # idx out of range
    assert lib.dcpt_mix_stride_bwd(p, p, p, 3, 1, p, p, None, 0, 2, 8, 8, 8, 2, 512, 64, 8, None) == 2   # no workspace
    assert lib.dcpt_grid_add(p, p, 4, 2, 2, 8, 8, 8, 2, None) == 1 and lib.dcpt_grid_add(p, p, 4, 2, 5, 8, 8, 8, 2, None) == 1
    assert lib.dcpt_grid_scatter(p, p, 4, 0, 4, 8, 6, 8, 4, None) == 1


def _model(network_g, hook_names, **over):
    from basicsr.models import build_model

    opt = dict(name="t", model_type="DCPTModel", scale=1, num_gpu=0, dist=False, rank=0, world_size=1, is_train=True, hook_names=hook_names,
               network_g=network_g, network_dc=dict(type="PromptIR_NoImg_DC", feature_dims=[8, 16, 32, 64], num_classes=3), path=dict(),
               train=dict(classify_opt=dict(type="CrossEntropyLoss", loss_weight=1.0), optim_g=dict(type="SGD", lr=0.0),
                          optim_dc=dict(type="SGD", lr=0.0)))
    opt.update(over)
    return build_model(opt)


@pytest.mark.parametrize("tag", sorted(NETS))
def test_hook_depth_defaults_to_the_reference_rule(tag):
    cfg, hook_names, want = NETS[tag]
    m = _model(dict(cfg), hook_names)
    assert m.hook_module_names == want and len(m.hooks) == len(want)
    m1 = _model(dict(cfg), hook_names, hook_depth=1)
    assert m1.hook_module_names == want
    # the rule as the parent commit wrote it
    assert want == [n for n, _ in m.net_g.named_modules() if hook_names in n and n.count(".") == 1]


def test_hook_depth_0_selects_swinir_decoder_rstbs():
    dc = dict(type="PromptIR_NoImg_DC", feature_dims=[36, 36, 36], num_classes=5, downsample=True)
    m = _model(dict(SWIN_TINY), "decode_layers", hook_depth=0, network_dc=dc)
    assert m.hook_module_names == ["decode_layers0", "decode_layers1", "decode_layers2"]
    assert [type(mod).__name__ for _, mod in m.select_hook_modules()] == ["RSTB"] * 3
    # containers are never hooked: 'encode_layers' is a ModuleList
    m2 = _model(dict(SWIN_TINY), "layers", hook_depth=0, network_dc=dc)
    assert m2.hook_module_names == ["decode_layers0", "decode_layers1", "decode_layers2"]
    with pytest.raises(ValueError):
        _model(dict(SWIN_TINY), "decode_layers", hook_depth=2, network_dc=dc)
    # a tap count that does not match the head is reported with the hooked modules' names, before the head runs
    m.hook_outputs = [torch.zeros(1, 36, 16, 16)] * 2
    m.lq = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="decode_layers0"):
        m._classify()


def _head(**kw):
    from basicsr.archs import build_network

    cfg = dict(type="PromptIR_NoImg_DC", feature_dims=[12, 12, 12], num_res_blocks=1, num_classes=5, downsample=True)
    cfg.update(kw)
    return build_network(cfg)


def test_head_builds_with_the_reference_state_dict(golden_dir):
    g = np.load(os.path.join(golden_dir, "dc_head_tokens.npz"))
    assert list(_head().state_dict().keys()) == [str(k) for k in g["a.keys"]]
    assert list(_head(feature_dims=[8, 16, 12], num_res_blocks=2).state_dict().keys()) == [str(k) for k in g["b.keys"]]
    plain = _head(downsample=False)
    assert list(plain.state_dict().keys()) == list(_head().state_dict().keys())


def test_head_accepts_tokens_and_maps_and_leaves_the_list_alone():
    net = _head()
    tokens = [torch.randn(2, 256, 12) for _ in range(3)]
    given = list(tokens)
    maps = net._token_maps(given)
    assert all(a is b for a, b in zip(given, tokens)), "the caller's list must not be rewritten"
    assert [s for _, s in maps] == [1, 2, 4]
    for (m, _), t in zip(maps, tokens):
        assert tuple(m.shape) == (2, 12, 16, 16) and m.data_ptr() == t.data_ptr()          # a view: no transpose pass
        assert torch.equal(m, t.transpose(1, 2).reshape(2, 12, 16, 16))                    # the reference's :627-631
    # 4-D channels_last maps, non-square allowed
    feats = [torch.randn(2, 12, 8, 24).contiguous(memory_format=torch.channels_last) for _ in range(3)]
    maps = net._token_maps(feats)
    assert [s for _, s in maps] == [1, 2, 4] and all(m is f for (m, _), f in zip(maps, feats))
    # the grid views of the stacked step (tap_split(..., stride=2**i)) are taken as they are
    views = [f[:, :, ::1 << i, ::1 << i] for i, f in enumerate(feats)]
    assert [s for _, s in net._token_maps(views)] == [1, 1, 1]
    # without a device there is no kernel to run: no eager fallback
    from dcpt_amd import _lib

    with pytest.raises(_lib.DcptHipError):
        net(None, tokens)


def test_head_input_errors():
    net = _head()
    with pytest.raises(ValueError, match="square"):
        net(None, [torch.zeros(1, 200, 12)] * 3)
    with pytest.raises(ValueError, match="multiple of 8"):
        net(None, [torch.zeros(1, 12, 12, 16)] * 3)        # H % 8 != 0 with three stages
    with pytest.raises(ValueError, match="multiple of 8"):
        net(None, [torch.zeros(1, 144, 12)] * 3)           # 12 x 12 tokens
    with pytest.raises(ValueError):
        net(None, [torch.zeros(1, 64, 12)] * 2)            # two taps for three stages
    with pytest.raises(ValueError):
        net(None, [torch.zeros(1, 64, 12), torch.zeros(1, 64, 8), torch.zeros(1, 64, 12)])   # channels
    with pytest.raises(ValueError):
        net(None, [torch.zeros(1, 12, 16, 16), torch.zeros(1, 12, 4, 4), torch.zeros(1, 12, 4, 4)])   # neither full nor its grid
    with pytest.raises((NotImplementedError, ValueError)):
        _head(feature_dims=[16, 16, 16], act_dtype="bf16")


def test_mix_and_tap_split_keep_their_default_signature():
    import inspect

    from dcpt_amd import functional as DF

    assert inspect.signature(DF.mix).parameters["stride"].default == 1
    assert inspect.signature(DF.tap_split).parameters["stride"].default == 1
    with pytest.raises(_import_err()):
        DF.mix(None, torch.zeros(1, 4, 4, 4), torch.ones(3), 1, stride=2)


def _import_err():
    from dcpt_amd import _lib

    return _lib.DcptHipError


def test_swinir_option_file():
    from basicsr.utils.options import yaml_load

    opt = yaml_load(os.path.join(ROOT, "options", "all_in_one", "train", "train_DCPT_SwinIR_5d.yml"))
    test = yaml_load(os.path.join(ROOT, "options", "all_in_one", "test", "test_SwinIR_5d.yml"))
    assert dict(opt["network_g"]) == dict(test["network_g"])
    assert opt["hook_names"] == "decode_layers" and opt["hook_depth"] == 0 and opt["model_type"] == "DCPTModel"
    dc = opt["network_dc"]
    assert dc["type"] == "PromptIR_NoImg_DC" and dc["feature_dims"] == [180, 180, 180] and dc["downsample"] is True
    assert all(v.get("allow_synthetic") for k, v in opt["datasets"].items() if k.startswith("train_"))


def test_golden_files_load(golden_dir):
    g = np.load(os.path.join(golden_dir, "dc_head_tokens.npz"))
    assert [str(c) for c in g["cases"]] == ["a", "b"]
    for tag, dims in (("a", [12, 12, 12]), ("b", [8, 16, 12])):
        assert g[f"{tag}.logits"].shape == (2, 5) and np.isfinite(float(g[f"{tag}.loss"]))
        for i, c in enumerate(dims):
            assert g[f"{tag}.df{i}"].shape == (2, 256, c)
        assert g[f"{tag}.g.mixing_weights"].shape == (3,) and f"{tag}.g.fc.weight" in g.files
        assert len(g[f"{tag}.g_names"]) == len(g[f"{tag}.g_l2"]) > 0
        # stage i only reads every 2**i-th token in both directions: the other gradients are exactly zero
        d2 = g[f"{tag}.df2"].reshape(2, 16, 16, -1)
        assert np.abs(d2[:, ::4, ::4]).max() > 0 and np.abs(d2[:, 1::4]).max() == 0 and np.abs(d2[:, :, 1::4]).max() == 0
    s = np.load(os.path.join(golden_dir, "dcpt_step_swinir.npz"))
    assert {"l_pix", "l_classify", "logits", "hooked", "g_names", "g_l2", "dc_names", "dc_l2"} <= set(s.files)
    assert [str(h) for h in s["hooked"]] == ["decode_layers0", "decode_layers1", "decode_layers2"]
    assert s["logits"].shape == (2, 5) and "dc.g.mixing_weights" in s.files and "g.g.conv_first.weight" in s.files
    for f in ("dc_head_tokens.npz", "dcpt_step_swinir.npz"):
        assert os.path.getsize(os.path.join(golden_dir, f)) < (1 << 20)
