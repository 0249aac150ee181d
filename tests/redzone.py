"""Does an entry point stay inside the buffers it was given?  ``with redzone() as rz: ...`` swaps the allocators of dcpt_amd.functional
(``_workspace``, ``_empty_nhwc``, ``_empty_nhwc_bf16``) for ones that hand out a fresh tensor of EXACTLY the requested size -- a view at
offset 0 of a larger buffer, with a guard of GUARD bytes of a fixed pattern behind it.  The product's grow-only workspace cache and the
caching allocator's rounding would otherwise give a tail-tile overrun slack that nobody reads.  On exit the context synchronises and
asserts that every guard still holds the pattern, naming the allocation site and the first damaged byte.

The pattern (0xFF bytes) is a NaN in fp32 and in bf16; with ``fill=True`` (default) the buffers themselves start as that pattern too, so a
kernel that reads workspace or output it never wrote produces NaNs instead of whatever the allocator last held."""
import contextlib
import sys

import torch

GUARD = 64 << 10      # bytes behind every allocation
PATTERN = 0xFF


class _Zone:
    def __init__(self, fill):
        self.fill = fill
        self.allocs = []   # (site, raw uint8 buffer, requested bytes)

    def raw(self, nbytes, dev, site):
        raw = torch.full((nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
        if not self.fill and nbytes:
            raw[:nbytes].zero_()
        self.allocs.append((site, raw, nbytes))
        return raw

    def workspace(self, dev, nbytes):
        return self.raw(int(nbytes), dev, _site())[: int(nbytes)]

    def nhwc(self, dtype):
        def empty(n, c, h, w, dev):
            esz = torch.empty((), dtype=dtype).element_size()
            nbytes = n * c * h * w * esz
            raw = self.raw(nbytes, dev, _site())
            return raw[:nbytes].view(dtype).as_strided((n, c, h, w), (h * w * c, 1, w * c, c))
        return empty

    @property
    def count(self):
        return len(self.allocs)

    def check(self):
        if self.allocs:
            torch.cuda.synchronize(self.allocs[0][1].device)
        for site, raw, nbytes in self.allocs:
            bad = raw[nbytes:] != PATTERN
            if bool(bad.any()):
                first = int(torch.nonzero(bad)[0])
                nbad = int(bad.sum())
                raise AssertionError(f"red zone: {nbad} guard byte(s) overwritten behind a {nbytes}-byte allocation of {site}, the first "
                                     f"at offset +{first} past its end (value 0x{int(raw[nbytes + first]):02x})")


def _site():
    f = sys._getframe(2)   # (the caller of the patched allocator)
    return f"{f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_code.co_name}:{f.f_lineno}"


@contextlib.contextmanager
def redzone(fill=True):
    """yields the zone: ``.count`` allocations were guarded (a test asserts > 0, or it checked nothing)"""
    from dcpt_amd import functional as DF

    zone = _Zone(fill)
    saved = DF._workspace, DF._empty_nhwc, DF._empty_nhwc_bf16
    DF._workspace, DF._empty_nhwc, DF._empty_nhwc_bf16 = zone.workspace, zone.nhwc(torch.float32), zone.nhwc(torch.bfloat16)
    try:
        yield zone
    finally:
        DF._workspace, DF._empty_nhwc, DF._empty_nhwc_bf16 = saved
    zone.check()
