"""Golden vectors of the reference's Bayer helpers (build container only; needs the reference tree).

    python tools/make_golden_mosaic.py [REFERENCE_ROOT]

Loads the reference's basicsr/utils/mosaic_util.py by file path (numpy and torch only) and writes tests/golden/mosaic.npz.  Per case:
    <tag>.cfa              mosaic_CFA_Bayer(...)[0] of each 8-bit image (uint8, B x H x W)
    <tag>.malvar64/.bilinear64   dm_matlab / dm in float64 on the 8-bit image's CFA (B x 3 x H x W): exact multiples of 1/16 and 1/4
    <tag>.malvar32/.bilinear32   dm_matlab / dm in float32 on the CFA of the keyed [0, 1] input itself
The inputs are keyed (dcpt_amd.keyed_init.keyed_input, tag ``mosaic.<tag>``, seed 0); the 8-bit image is rint(255 x).  Arrays only.
Single-threaded CPU, so a rerun reproduces the file bit for bit."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dcpt_amd.keyed_init import keyed_input  # noqa: E402
from oracle import ref_import  # noqa: E402  (REF: where the reference tree lives)

OUT = os.path.join(ROOT, "tests", "golden", "mosaic.npz")
CASES = {"4x4": (1, 3, 4, 4), "6x8": (1, 3, 6, 8), "16x16": (1, 3, 16, 16), "34x66": (1, 3, 34, 66), "b2_10x12": (2, 3, 10, 12)}


def pack(cfa):
    """(B, H, W) -> the (B, 4, H / 2, W / 2) phases the reference's demosaics take"""
    return torch.stack([cfa[:, 0::2, 0::2], cfa[:, 0::2, 1::2], cfa[:, 1::2, 0::2], cfa[:, 1::2, 1::2]], dim=1)


def main():
    torch.set_num_threads(1)
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_import.REF
    spec = importlib.util.spec_from_file_location("_ref_mosaic_util", os.path.join(ref_root, "basicsr", "utils", "mosaic_util.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for tag, shape in CASES.items():
        x = keyed_input(f"mosaic.{tag}", shape)
        u8 = torch.round(x * 255).to(torch.uint8)
        cfa = np.stack([ref.mosaic_CFA_Bayer(im.permute(1, 2, 0).numpy())[0] for im in u8])
        out[f"{tag}.cfa"] = cfa
        p64 = pack(torch.from_numpy(cfa).double())
        out[f"{tag}.malvar64"], out[f"{tag}.bilinear64"] = ref.dm_matlab(p64).numpy(), ref.dm(p64).numpy()
        mask = np.stack(ref.masks_CFA_Bayer(shape[2:]), axis=0)
        p32 = pack((x * torch.from_numpy(mask).float()).sum(1))
        out[f"{tag}.malvar32"], out[f"{tag}.bilinear32"] = ref.dm_matlab(p32).numpy(), ref.dm(p32).numpy()
        d = float((ref.dm_matlab(p32).double() - ref.dm_matlab(p32.double())).abs().max())
        print(f"{tag} {shape}: dm_matlab in fp32 against its float64 form {d:.3e}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
