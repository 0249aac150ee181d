"""The cases the Poisson-noise tests share (tests/test_poisson_cpu.py checks the restatement on them, tests/test_gpu_poisson.py the
kernels): name -> (shape, scale per image, key per image, gray per image or None).  Inputs are ``keyed_input(..., lo=-0.1, hi=1.1)`` (some
samples beyond the clamp) unless the name is in SPECIAL.

One element (U = 1, vals = 1); one gray pixel of three channels (a partial quad); 105 elements per image: the second image starts 4 bytes
off a 16-byte boundary, ends in a partial quad and is gray (35 pixels per plane, planes 1 and 2 misaligned); one channel, one gray image;
1683 elements per image with scale 0 / 0.5 / 1 and a gray image (561 pixels per plane: odd); 12480 elements = 3120 quads per image: 4 chunks
of the level pass (a chunk is 4096 elements) and 13 workgroups of the sampler (256 lanes of 4 elements), and U reaches 256; palette
images of exactly 16, 17, 255 and 256 levels (vals 16, 32, 256, 256); an all-zero image (lambda = 0, k = 0 everywhere)."""
import numpy as np
import torch

from dcpt_amd.keyed_init import keyed_input

CASES = {
    "1x1x1x1": ((1, 1, 1, 1), [1.0], [11], None),
    "1x3x1x1": ((1, 3, 1, 1), [1.0], [12], [1]),
    "2x3x5x7": ((2, 3, 5, 7), [1.0, 0.75], [13, (1 << 63) - 1], [0, 1]),
    "3x1x6x6": ((3, 1, 6, 6), [0.25, 1.0, 2.0], [14, 15, -16], [1, 0, 0]),
    "3x3x17x33": ((3, 3, 17, 33), [0.0, 0.5, 1.0], [(3 << 32) | 17, 18, 0x0123456789ABCDEF], [0, 1, 0]),
    "2x3x64x65": ((2, 3, 64, 65), [1.0, 0.5], [20, 21], None),
    "palettes": ((4, 3, 10, 11), [1.0, 1.0, 1.0, 1.0], [30, 31, 32, 33], None),
    "zeros": ((1, 3, 4, 5), [1.0], [40], [0]),
}
SPECIAL = ("palettes", "zeros")
PALETTE_LEVELS = (16, 17, 255, 256)


def palette(tag, n_levels, shape):
    """an image of ``shape`` whose values are l / 255 (fp32) for exactly ``n_levels`` distinct l, each present, in a keyed order"""
    rs = np.random.RandomState(n_levels * 1000 + len(tag))
    chosen = rs.permutation(256)[:n_levels]
    size = int(np.prod(shape))
    assert size >= n_levels
    lev = chosen[np.arange(size) % n_levels]
    rs.shuffle(lev)
    return torch.from_numpy((lev.astype(np.float64) / 255.0).astype(np.float32).reshape(shape))


def case_args(name):
    shape, scale, key, gray = CASES[name]
    if name == "palettes":
        x = torch.stack([palette(name, n, shape[1:]) for n in PALETTE_LEVELS])
    elif name == "zeros":
        x = torch.zeros(shape)
    else:
        x = keyed_input(f"gpupoisson.{name}", shape, lo=-0.1, hi=1.1)
    return (x, torch.tensor(scale, dtype=torch.float32), torch.tensor(key, dtype=torch.int64),
            None if gray is None else torch.tensor(gray, dtype=torch.int32))
