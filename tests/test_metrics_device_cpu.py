"""CPU: the C ABI of the device-side validation metrics (include/dcpt_hip.h dcpt_imgmetric*, dcpt_amd/csrc/metrics.hip) as far as it goes
without a device -- the symbols, the workspace query, the argument errors (reported before any launch), and the refusal of CPU tensors."""
import pytest
import torch

Y, SSIM, RANGE1 = 1, 2, 4   # DCPT_METRIC_* of the header


def _lib():
    from dcpt_amd import _lib

    return _lib, _lib.load()


def test_symbols_are_exported_and_bound():
    L, lib = _lib()
    for name in ("dcpt_imgmetric_ws_bytes", "dcpt_imgmetric"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.dcpt_abi_version() == L.ABI_VERSION


def test_workspace_query_needs_no_device_and_grows():
    from dcpt_amd import functional as DF

    _, lib = _lib()
    ws = lib.dcpt_imgmetric_ws_bytes
    base = ws(1, 1, 256, 256, 0, SSIM)   # (128 tiles: past the 256-byte granule of a workspace row)
    assert base > 0
    assert ws(4, 1, 256, 256, 0, SSIM) > base and ws(1, 3, 256, 256, 0, SSIM) > base
    assert ws(1, 1, 512, 256, 0, SSIM) > base and ws(1, 1, 256, 512, 0, SSIM) > base
    assert ws(1, 3, 256, 256, 0, SSIM | Y) == base            # luma scores one channel
    assert ws(1, 3, 1080, 2048, 0, SSIM) < 1 << 20   # (tiny: two 8-byte partials per tile)
    # the tile edges Python exports are the kernel's: one more map position than a tile holds is one more tile (two 8-byte partials, 256-byte rows)
    th, tw = DF.METRIC_TILE
    rows = [ws(1, 1, 10 + 32 * th + d, 11, 0, SSIM) for d in (0, 1)]
    cols = [ws(1, 1, 11, 10 + 32 * tw + d, 0, SSIM) for d in (0, 1)]
    assert rows[1] - rows[0] == 2 * 256 and cols[1] - cols[0] == 2 * 256
    assert ws(1, 1, 10 + 31 * th + 1, 11, 0, SSIM) == rows[0] and ws(1, 1, 11, 10 + 31 * tw + 1, 0, SSIM) == cols[0]
    assert ws(1, 1, 8, 8, 0, 0) > 0 and ws(1, 1, 8, 8, 0, SSIM) == 0   # PSNR alone has no 11-pixel minimum


@pytest.mark.parametrize("what, args, word", [
    ("null images", (None, None, 1, 1, 1, 1 << 12, 1, 3, 32, 32, 0, SSIM), b"null"),
    ("null ssim_out with SSIM", (1, 1, 1, None, 1, 1 << 12, 1, 3, 32, 32, 0, SSIM), b"null"),
    ("C = 2", (1, 1, 1, 1, 1, 1 << 12, 1, 2, 32, 32, 0, SSIM), b"C must be 1 or 3"),
    ("cropped height 10 with SSIM", (1, 1, 1, 1, 1, 1 << 12, 1, 3, 16, 32, 3, SSIM), b"at least 11 x 11"),
    ("nothing left after the crop", (1, 1, 1, 1, 1, 1 << 12, 1, 3, 16, 32, 8, 0), b"nothing left"),
    ("unknown image_range flag", (1, 1, 1, 1, 1, 1 << 12, 1, 3, 32, 32, 0, SSIM | 8), b"unknown flag"),
    ("undersized workspace", (1, 1, 1, 1, 1, 8, 1, 3, 32, 32, 0, SSIM), b"workspace too small"),
    ("null workspace", (1, 1, 1, 1, None, 0, 1, 3, 32, 32, 0, SSIM), b"workspace too small"),
])
def test_bad_arguments_are_reported_before_any_launch(what, args, word):
    """(the pointers are the integer 1: a launch would fault, and this machine has no device to launch on -- an error return with the
    telling message is only possible if the check came first)"""
    _, lib = _lib()
    rc = lib.dcpt_imgmetric(*args, None)
    assert rc != 0, what
    assert word in lib.dcpt_last_error(), (what, lib.dcpt_last_error())


def test_cpu_tensors_are_refused():
    L, _ = _lib()
    from basicsr.metrics import METRIC_REGISTRY, MetricSums, calculate_psnr_device, calculate_ssim_device
    from dcpt_amd import functional as DF

    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    with pytest.raises(L.DcptHipError):
        DF.image_metric_sums(a, b)
    with pytest.raises(L.DcptHipError):
        calculate_psnr_device(a, b, 0)
    with pytest.raises(L.DcptHipError):
        MetricSums().add(a, b)
    assert METRIC_REGISTRY.get("calculate_psnr_device") is calculate_psnr_device
    assert METRIC_REGISTRY.get("calculate_ssim_device") is calculate_ssim_device
    with pytest.raises(ValueError):
        MetricSums(image_range=65535)
    with pytest.raises(ValueError):
        MetricSums(input_order="BHWC")
