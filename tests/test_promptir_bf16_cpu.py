"""CPU: PromptIR act_dtype="bf16" construction, the wide-head MDTA workspace queries and the bf16 prompt-mix entry points' argument
errors (no GPU needed)."""
import pytest
import torch

from basicsr.archs import build_network
from dcpt_amd import _lib

P_CFG = dict(num_blocks=[1, 1, 1, 1], num_refinement_blocks=1)


def test_bf16_build_same_state_dict():
    a = build_network(dict(type="PromptIR", **P_CFG))
    b = build_network(dict(type="PromptIR", act_dtype="bf16", **P_CFG))
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert all(sa[k].shape == sb[k].shape and sb[k].dtype == torch.float32 for k in sa)
    assert a.act_dtype == "fp32" and b.act_dtype == "bf16"
    assert b.noise_level3.bf16 and b.patch_embed.bf16 and b.refinement[0].bf16
    assert not a.noise_level3.bf16 and not a.patch_embed.bf16


def test_bad_act_dtype():
    with pytest.raises(ValueError):
        build_network(dict(type="PromptIR", act_dtype="fp16", **P_CFG))


def test_cpu_tensor_raises():
    net = build_network(dict(type="PromptIR", act_dtype="bf16", **P_CFG))
    with pytest.raises(_lib.DcptHipError):
        net(torch.rand(1, 3, 16, 16))


@pytest.mark.parametrize("C,heads", [(704, 4), (208, 2), (256, 1)])
@pytest.mark.parametrize("b", [0, 1, 2, 3])
def test_wide_head_ws_queries(C, heads, b):
    # head widths 176, 104 and 256: beyond the 96 channels of the narrow per-head kernels
    lib = _lib.load()
    n = lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, C, heads, b)
    assert n > 0
    ch, P = C // heads, 16 * 16
    assert n >= 2 * heads * ((P + 255) // 256) * ch * ch * 4    # the fp32 Gram slabs of every (image, head)


def test_ws_queries_reject():
    lib = _lib.load()
    assert lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 264, 1, 0) == 0     # head width 264 > 256
    assert lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 48, 12, 0) == 0     # head width 4
    assert lib.dcpt_mdta_bf16_ws_bytes(2, 16, 16, 1056, 4, 0) == 0    # C > 1024
    assert lib.dcpt_abi_version() == 16
    # the GDFN of the 704-channel block (hidden int(704 * 2.66) = 1872) at PromptIR's level-3 maps of 128 / 64 patches
    for hw in (32, 16):
        assert lib.dcpt_gdfn_bf16_ws_bytes(2, hw, hw, 704, 1872, 1) > 0


def _err(rc):
    assert rc != 0
    return _lib.load().dcpt_last_error().decode()


def test_prompt_mix_bf16_argument_errors():
    lib = _lib.load()
    fake = 256   # non-null dummies (never dereferenced: the argument checks come first)
    assert "null" in _err(lib.dcpt_prompt_mix_fwd_bf16(None, fake, fake, fake, 1, 5, 64, 8, 4, 4, None))
    assert "null" in _err(lib.dcpt_prompt_mix_fwd_bf16(fake, fake, fake, None, 1, 5, 64, 8, 4, 4, None))
    assert "bad shape" in _err(lib.dcpt_prompt_mix_fwd_bf16(fake, fake, fake, fake, 1, 5, 36, 8, 4, 4, None))    # D % 8
    assert "bad shape" in _err(lib.dcpt_prompt_mix_fwd_bf16(fake, fake, fake, fake, 1, 9, 64, 8, 4, 4, None))    # prompt_len > 8
    assert "bad shape" in _err(lib.dcpt_prompt_mix_fwd_bf16(fake, fake, fake, fake, 0, 5, 64, 8, 4, 4, None))    # B
    assert "null" in _err(lib.dcpt_prompt_mix_bwd_bf16(fake, fake, fake, None, fake, fake, 1 << 20, 1, 5, 64, 8, 4, 4, None))
    assert "bad shape" in _err(lib.dcpt_prompt_mix_bwd_bf16(fake, fake, fake, fake, fake, fake, 1 << 20, 1, 5, 36, 8, 4, 4, None))
    assert "workspace" in _err(lib.dcpt_prompt_mix_bwd_bf16(fake, fake, fake, fake, fake, None, 0, 1, 5, 64, 8, 4, 4, None))
    assert "workspace" in _err(lib.dcpt_prompt_mix_bwd_bf16(fake, fake, fake, fake, fake, fake, 16, 1, 5, 64, 8, 4, 4, None))
