"""CPU: the C ABI and the Python plumbing of the TLSC block in bf16 storage (include/dcpt_hip.h dcpt_nafblock_local_fwd_bf16*,
dcpt_box_mean_bf16*; dcpt_amd/csrc/nafblock_bf16.hip, tlsc_bf16.hip) as far as they go without a device."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcpt_nafblock_local_fwd_bf16_ws_bytes", "dcpt_nafblock_local_fwd_bf16", "dcpt_box_mean_bf16_ws_bytes", "dcpt_box_mean_bf16")
TINY = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 2], dec_blk_nums=[1, 1, 1, 1])


def _header_argc(name):
    text = open(os.path.join(ROOT, "include", "dcpt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/dcpt_hip.h"
    args = m.group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


def test_symbols_in_header_signatures_and_library():
    from dcpt_amd import _lib, build

    lib_path = build.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == _header_argc(name), name
        assert re.search(r"\sT\s+" + name + r"$", exported, flags=re.M), f"{name} is not exported"
        assert getattr(lib, name).argtypes is not None
    assert lib.dcpt_abi_version() == _lib.ABI_VERSION == 16
    text = open(os.path.join(ROOT, "include", "dcpt_hip.h")).read()
    assert "arch_util.py:378-396" in text and "nafnet_arch.py:277-288" in text   # the prototypes cite the reference


def test_workspace_queries_need_no_device():
    from dcpt_amd import _lib

    lib = _lib.load()
    a = lib.dcpt_nafblock_local_fwd_bf16_ws_bytes(2, 12, 20, 64, 5, 5)
    assert a > 0 and a % 256 == 0
    assert lib.dcpt_nafblock_local_fwd_bf16_ws_bytes(2, 12, 20, 60, 5, 5) == 0   # C % 8
    # the box mean's fp32 row sums: B H (W - k2 + 1) C floats (in 256-byte units), the window clamped to the map
    assert lib.dcpt_box_mean_bf16_ws_bytes(1, 4, 10, 8, 3, 3) == 4 * 8 * 8 * 4
    assert lib.dcpt_box_mean_bf16_ws_bytes(1, 4, 10, 8, 3, 99) == 256   # 4 * 1 * 8 floats = 128 bytes
    assert lib.dcpt_box_mean_bf16_ws_bytes(1, 4, 10, 12, 3, 3) == 0


def test_argument_errors_launch_nothing():
    from dcpt_amd import _lib

    lib = _lib.load()
    assert lib.dcpt_nafblock_local_fwd_bf16(None, None, 0, None, None, None, 0, 1, 4, 4, 8, 2, 2, None) == 1   # DCPT_ERR_ARG
    assert b"null" in lib.dcpt_last_error()
    assert lib.dcpt_box_mean_bf16(None, None, None, 0, 1, 4, 4, 8, 2, 2, None) == 1


@pytest.mark.parametrize("mode", ["bf16", "bf16_tail32", "bf16_edge32"])
def test_nafnet_tlsc_constructs_in_bf16_modes(mode):
    from basicsr.archs import build_network
    from basicsr.archs.nafnet_arch import NAFBlock

    net = build_network(dict(type="NAFNet", train_size=(1, 3, 16, 16), act_dtype=mode, **TINY))
    blocks = [m for m in net.modules() if isinstance(m, NAFBlock)]
    assert len(blocks) == 10 and all(m.local_sca() for m in blocks)
    n32 = {"bf16": 0, "bf16_tail32": 1, "bf16_edge32": 2}[mode]
    assert sum(not m.act_bf16 for m in blocks) == n32
    # local blocks read the same weight pack as the global ones (dcpt_nafblock_local_fwd_bf16 takes it), so none is left out of the
    # network's pack list.  The list is built on the first device forward: tests/test_gpu_tlsc_bf16.py::test_network_vs_reference_golden
    # asserts its length there; without a device it does not exist yet
    assert "_bf16_blocks" not in net.__dict__


def test_no_cpu_fallback():
    from dcpt_amd import _lib
    from dcpt_amd import functional as DF

    c = 8
    P = {k: torch.zeros(1) for k in _lib.PARAM_FIELDS}
    x = torch.zeros(1, c, 6, 6, dtype=torch.bfloat16)
    with torch.no_grad():
        with pytest.raises(_lib.DcptHipError):
            DF.nafblock_local_bf16(x, P, 2, 2)
        with pytest.raises(_lib.DcptHipError):
            DF.box_mean_bf16(x, 2, 2)
    with pytest.raises(NotImplementedError):   # inference only, like nafblock_local
        DF.nafblock_local_bf16(x.requires_grad_(False), {k: torch.zeros(1, requires_grad=True) for k in _lib.PARAM_FIELDS}, 2, 2)
