"""CPU: SwinIR's super-resolution forms and the 3conv residual have the reference's state-dict layout (against the key fixtures of the real
reference, tools/make_golden_swinir_sr.py), the combinations off the path raise, the new C-ABI entry points (dcpt_conv3x3_act_*,
dcpt_up2_conv3x3_act_*, dcpt_conv3x3_ps_out_*, dcpt_conv3conv_res_*) answer workspace queries and report bad arguments without a GPU, and
there is no CPU fallback."""
import os

import numpy as np
import pytest
import torch

BODY = dict(img_size=64, window_size=8, mlp_ratio=2.0, depths=[6] * 6)
KEY_NETS = [("classical_x4_c180", dict(embed_dim=180, num_heads=[6] * 6, upsampler="pixelshuffle", upscale=4)),
            ("lightweight_x2_c60", dict(embed_dim=60, num_heads=[6] * 6, upsampler="pixelshuffledirect", upscale=2)),
            ("realworld_x4_c240_3conv", dict(embed_dim=240, num_heads=[8] * 6, upsampler="nearest+conv", upscale=4, resi_connection="3conv"))]


def _build(**kw):
    import basicsr.archs  # noqa: F401  (registers the archs)
    from basicsr.utils.registry import ARCH_REGISTRY

    return ARCH_REGISTRY.get("SwinIR")(**kw)


@pytest.mark.parametrize("tag,kw", KEY_NETS)
def test_state_dict_matches_reference(golden_dir, tag, kw):
    g = np.load(os.path.join(golden_dir, f"swinir_sr_key_{tag}.npz"))
    net = _build(**BODY, **kw)
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(g["key_shapes"])
    assert sum(p.numel() for p in net.parameters()) == int(g["n_params"])
    net.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)


def test_module_keys_of_each_form():
    tiny = dict(img_size=64, window_size=8, embed_dim=48, depths=[2] * 6, num_heads=[6] * 6)
    tail = lambda net: {k.rsplit(".", 1)[0] for k in net.state_dict() if "layers" not in k and not k.startswith(("conv_first", "patch_embed", "norm"))}   # noqa: E731
    assert tail(_build(upsampler="pixelshuffle", upscale=8, **tiny)) == {"conv_after_body", "conv_before_upsample.0", "upsample.0", "upsample.2",
                                                                         "upsample.4", "conv_last"}
    assert tail(_build(upsampler="pixelshuffle", upscale=3, **tiny)) == {"conv_after_body", "conv_before_upsample.0", "upsample.0", "conv_last"}
    assert tail(_build(upsampler="pixelshuffledirect", upscale=3, **tiny)) == {"conv_after_body", "upsample.0"}
    two = _build(upsampler="nearest+conv", upscale=2, resi_connection="3conv", **tiny)
    assert tail(two) == {"conv_after_body.0", "conv_after_body.2", "conv_after_body.4", "conv_before_upsample.0", "conv_up1", "conv_hr", "conv_last"}
    assert {"encode_layers.0.conv.0.weight", "encode_layers.0.conv.2.weight", "decode_layers2.conv.4.bias"} <= set(two.state_dict())
    assert tuple(two.state_dict()["conv_after_body.2.weight"].shape) == (12, 12, 1, 1)
    assert tuple(_build(upsampler="pixelshuffledirect", upscale=3, **tiny).state_dict()["upsample.0.weight"].shape) == (27, 48, 3, 3)


def test_combinations_off_the_path_raise():
    with pytest.raises(NotImplementedError, match="nearest"):
        _build(upsampler="nearest+conv", upscale=3)
    with pytest.raises(NotImplementedError, match="pixelshuffledirect"):
        _build(upsampler="pixelshuffledirect", upscale=8)
    with pytest.raises(NotImplementedError, match="240"):
        _build(resi_connection="3conv")   # the default width 180: Cq = 45
    with pytest.raises(NotImplementedError):
        _build(upsampler="bicubic", upscale=2)
    with pytest.raises(NotImplementedError):
        _build(upsampler="pixelshuffle", upscale=5)


@pytest.mark.parametrize("kw", [dict(upsampler="pixelshuffle", upscale=2), dict(upsampler="pixelshuffledirect", upscale=3),
                                dict(upsampler="nearest+conv", upscale=2), dict(resi_connection="3conv")])
def test_no_cpu_fallback(kw):
    from dcpt_amd import _lib

    net = _build(img_size=64, window_size=8, embed_dim=48, depths=[2] * 6, num_heads=[6] * 6, **kw)
    with pytest.raises(_lib.DcptHipError):
        net(torch.zeros(1, 3, 8, 8))


def test_nodes_refuse_cpu_tensors_and_bad_shapes():
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    x, w, b = torch.zeros(1, 8, 4, 4), torch.zeros(12, 8, 3, 3), torch.zeros(12)
    for fn in (lambda: DF.conv3x3_act(x, w, b, 0.2), lambda: DF.up2_conv3x3_act(x, torch.zeros(8, 8, 3, 3), torch.zeros(8)),
               lambda: DF.conv3x3_ps_out(x, w, b, 2),
               lambda: DF.conv3conv_res(torch.zeros(1, 16, 4, 4), torch.zeros(4, 16, 3, 3), torch.zeros(4), torch.zeros(4, 4, 1, 1), torch.zeros(4),
                                        torch.zeros(16, 4, 3, 3), torch.zeros(16), torch.zeros(1, 16, 4, 4))):
        with pytest.raises(_lib.DcptHipError):
            fn()


def test_workspace_queries_need_no_gpu():
    from dcpt_amd import _lib

    lib = _lib.load()
    M = 8 * 64 * 64
    f, b = lib.dcpt_conv3x3_act_ws_bytes(8, 64, 64, 180, 64, 0), lib.dcpt_conv3x3_act_ws_bytes(8, 64, 64, 180, 64, 1)
    assert f >= 9 * 180 * 64 * 4 and b >= f + M * 64 * 4            # packed weights; + the masked dy
    f, b = lib.dcpt_up2_conv3x3_act_ws_bytes(8, 64, 64, 64, 0), lib.dcpt_up2_conv3x3_act_ws_bytes(8, 64, 64, 64, 1)
    assert f >= 9 * 64 * 64 * 4 and b >= f + 2 * 4 * M * 64 * 4       # + the masked dy and the dgrad on the 2H x 2W grid
    f, b = lib.dcpt_conv3x3_ps_out_ws_bytes(8, 64, 64, 60, 3, 3, 0), lib.dcpt_conv3x3_ps_out_ws_bytes(8, 64, 64, 60, 3, 3, 1)
    assert f >= M * 28 * 4 and b > f                                  # the conv rows, padded from 27 to 28 columns
    f, b = lib.dcpt_conv3conv_res_ws_bytes(8, 64, 64, 240, 0), lib.dcpt_conv3conv_res_ws_bytes(8, 64, 64, 240, 1)
    assert f >= 2 * M * 60 * 4 and b > f
    # unsupported arguments
    assert lib.dcpt_conv3x3_act_ws_bytes(1, 8, 8, 30, 64, 0) == 0 and lib.dcpt_conv3x3_act_ws_bytes(1, 8, 8, 64, 30, 1) == 0
    assert lib.dcpt_conv3x3_act_ws_bytes(0, 8, 8, 64, 64, 0) == 0 and lib.dcpt_up2_conv3x3_act_ws_bytes(1, 8, 8, 30, 0) == 0
    assert lib.dcpt_conv3x3_ps_out_ws_bytes(1, 8, 8, 60, 3, 5, 0) == 0 and lib.dcpt_conv3x3_ps_out_ws_bytes(1, 8, 8, 60, 3, 1, 0) == 0
    assert lib.dcpt_conv3x3_ps_out_ws_bytes(1, 8, 8, 60, 5, 2, 0) == 0 and lib.dcpt_conv3x3_ps_out_ws_bytes(1, 8, 8, 30, 3, 2, 0) == 0
    assert lib.dcpt_conv3conv_res_ws_bytes(1, 8, 8, 180, 0) == 0 and lib.dcpt_conv3conv_res_ws_bytes(1, 8, 8, 12, 1) == 0


def test_bad_arguments_are_reported_not_crashed():
    from dcpt_amd import _lib

    lib = _lib.load()
    err = lib.dcpt_last_error
    assert lib.dcpt_conv3x3_act_fwd(1, None, 1, 1, None, 0, 1, 8, 8, 64, 64, 0.2, None) != 0 and b"null" in err()
    assert lib.dcpt_conv3x3_act_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 30, 64, 0.2, None) != 0 and b"multiples of 4" in err()
    assert lib.dcpt_conv3x3_act_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 64, 64, -0.5, None) != 0 and b"slope" in err()
    assert lib.dcpt_conv3x3_act_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 64, 64, 0.2, None) != 0 and b"workspace" in err()
    assert lib.dcpt_conv3x3_act_bwd(1, 1, None, 1, 1, 1, 1, None, 0, 1, 8, 8, 64, 64, 0.2, None) != 0 and b"null" in err()
    assert lib.dcpt_conv3x3_act_bwd(1, 1, 1, 1, 1, 1, 1, None, 0, 1, 8, 8, 64, 64, 0.2, None) != 0 and b"workspace" in err()
    assert lib.dcpt_up2_conv3x3_act_fwd(1, 1, None, 1, None, 0, 1, 8, 8, 64, 0.2, None) != 0 and b"null" in err()
    assert lib.dcpt_up2_conv3x3_act_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 64, 0.2, None) != 0 and b"workspace" in err()
    assert lib.dcpt_up2_conv3x3_act_bwd(1, 1, 1, 1, None, 1, 1, None, 0, 1, 8, 8, 64, 0.2, None) != 0 and b"null" in err()
    assert lib.dcpt_conv3x3_ps_out_fwd(1, 1, 1, None, None, 0, 1, 8, 8, 60, 3, 2, None) != 0 and b"null" in err()
    assert lib.dcpt_conv3x3_ps_out_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 60, 3, 5, None) != 0 and b"r 2..4" in err()
    assert lib.dcpt_conv3x3_ps_out_fwd(1, 1, 1, 1, None, 0, 1, 8, 8, 60, 3, 3, None) != 0 and b"workspace" in err()
    assert lib.dcpt_conv3x3_ps_out_bwd(None, 1, 1, 1, 1, 1, None, 0, 1, 8, 8, 60, 3, 2, None) != 0 and b"null" in err()
    p, g = _lib.Conv3convParams(*([1] * 6)), _lib.Conv3convParams(*([1] * 6))
    assert lib.dcpt_conv3conv_res_fwd(None, 1, 1, 1, None, None, None, 0, 1, 8, 8, 64, None) != 0 and b"null" in err()
    assert lib.dcpt_conv3conv_res_fwd(_lib.Conv3convParams(1, 1, None, 1, 1, 1), 1, 1, 1, None, None, None, 0, 1, 8, 8, 64, None) != 0 and b"null" in err()
    assert lib.dcpt_conv3conv_res_fwd(p, 1, 1, 1, 1, None, None, 0, 1, 8, 8, 64, None) != 0 and b"both saved maps" in err()
    assert lib.dcpt_conv3conv_res_fwd(p, 1, 1, 1, None, None, None, 0, 1, 8, 8, 180, None) != 0 and b"multiple of 16" in err()
    assert lib.dcpt_conv3conv_res_fwd(p, 1, 1, 1, None, None, None, 0, 1, 8, 8, 64, None) != 0 and b"workspace" in err()
    assert lib.dcpt_conv3conv_res_bwd(p, g, 1, 1, None, 1, 1, None, 0, 1, 8, 8, 64, None) != 0 and b"null" in err()
    assert lib.dcpt_conv3conv_res_bwd(p, _lib.Conv3convParams(1, 1, 1, 1, 1, None), 1, 1, 1, 1, 1, None, 0, 1, 8, 8, 64, None) != 0 and b"gradient" in err()
    assert lib.dcpt_conv3conv_res_bwd(p, g, 1, 1, 1, 1, 1, None, 0, 1, 8, 8, 64, None) != 0 and b"workspace" in err()
