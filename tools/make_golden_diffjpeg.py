"""Golden vectors of the reference DiffJPEG (build container only; needs the reference tree).

    python tools/make_golden_diffjpeg.py [REFERENCE_ROOT]

Loads the reference's basicsr/utils/diffjpeg.py by file path (its package import needs cv2), runs ``DiffJPEG(differentiable=False)`` and
``DiffJPEG(True)`` on the CPU on keyed inputs (dcpt_amd.keyed_init.keyed_input) and writes tests/golden/diffjpeg.npz: the outputs only,
the inputs being keyed.  Single-threaded CPU float32, so a rerun reproduces the file bit for bit.

A committed vector must be free of contested roundings.  The module is loaded a second time and run in float64; for every key the
quantised coefficients of the fp32 run, of that float64 run and of tests/jpeg_restatement.py must be the same numbers, and no pre-round
value of the restatement may lie within 1e-6 of a tie.  A key that fails is replaced by the next seed of the same case, and the seed that
was used is stored with the vector.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_restatement as R  # noqa: E402
from dcpt_amd.keyed_init import keyed_input  # noqa: E402
from oracle import ref_import  # noqa: E402  (REF: where the reference tree lives)

OUT = os.path.join(ROOT, "tests", "golden", "diffjpeg.npz")
# tag -> ((B, C, H, W), quality: one number, or one per image)
CASES = {
    "mb3x2": ((2, 3, 24, 40), [10.0, 75.0]),      # ragged on both axes, both factor branches in one batch
    "one_mb": ((1, 3, 16, 16), 50),               # one macroblock, the branch point, a Python-number quality
    "ragged": ((2, 3, 17, 33), [30.0, 90.0]),
    "grey": ((2, 1, 24, 24), [20.0, 95.0]),
    "pixel": ((1, 3, 1, 1), 30),
}


def load_reference(ref_root: str, name: str):
    """a private copy of the module: its tables are module-level parameters, so the float64 run needs a copy of its own"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, "basicsr", "utils", "diffjpeg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _quality(q, dtype):
    return q if isinstance(q, (int, float)) else torch.tensor(q, dtype=dtype)


def _coefficients(mod, codec, x, q):
    """the quantised coefficients of ``codec.compress`` on the padded batch, as DiffJPEG.forward computes them"""
    factor = _quality(q, x.dtype)
    if isinstance(factor, (int, float)):
        factor = mod.quality_to_factor(factor)
    else:
        for i in range(factor.size(0)):
            factor[i] = mod.quality_to_factor(factor[i])
    _, c, h, w = x.shape
    if c == 1:
        x = x.repeat(1, 3, 1, 1)
    x = F.pad(x, (0, -w % 16, 0, -h % 16))
    return [t.reshape(-1) for t in codec.compress(x, factor=factor)]


def main():
    torch.set_num_threads(1)
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_import.REF
    m32, m64 = load_reference(ref_root, "_ref_diffjpeg_f32"), load_reference(ref_root, "_ref_diffjpeg_f64")
    out = {}
    with torch.no_grad():
        hard32, soft32 = m32.DiffJPEG(differentiable=False), m32.DiffJPEG(differentiable=True)
        hard64 = m64.DiffJPEG(differentiable=False).double()
        soft64 = m64.DiffJPEG(differentiable=True).double()
        for tag, (shape, q) in CASES.items():
            for seed in range(16):
                x = keyed_input(f"diffjpeg.{tag}", shape, seed=seed)
                c32, c64 = _coefficients(m32, hard32, x, q), _coefficients(m64, hard64, x.double(), q)
                res = R.diffjpeg(x, _quality(q, torch.float32))
                cr = [torch.round(t).reshape(-1) for t in (res.t_y, res.t_cb, res.t_cr)]   # (the reference's block order: row-major)
                same = all(torch.equal(a.double(), b) and torch.equal(b, c) for a, b, c in zip(c32, c64, cr))
                if same and not R.tie_macroblocks(res, 1e-6):
                    break
                print(f"{tag}: seed {seed} holds a contested rounding, trying the next")
            else:
                raise SystemExit(f"{tag}: no uncontested key among 16 seeds")
            y_hard, y_soft = hard32(x, _quality(q, torch.float32)), soft32(x, _quality(q, torch.float32))
            d64 = max(float((y_hard.double() - hard64(x.double(), _quality(q, torch.float64))).abs().max()),
                      float((y_soft.double() - soft64(x.double(), _quality(q, torch.float64))).abs().max()))
            dr = max(float((y_hard.double() - res.y).abs().max()),
                     float((y_soft.double() - R.diffjpeg(x, _quality(q, torch.float32), differentiable=True).y).abs().max()))
            print(f"{tag} {shape} q={q} seed {seed}: fp32 against its float64 form {d64:.3e}, against the restatement {dr:.3e}")
            assert dr <= 2e-6, (tag, dr)
            out[f"{tag}.hard"], out[f"{tag}.soft"] = y_hard.numpy(), y_soft.numpy()
            out[f"{tag}.seed"] = np.int64(seed)
            out[f"{tag}.quality"] = np.asarray(q, dtype=np.float32)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
