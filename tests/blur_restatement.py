"""The float64 numpy restatement of the blur kernel (include/dcpt_hip.h dcpt_filter2d_fwd) and of ``USMSharp.forward`` around it, written
from the header's statement alone: the image reflect-padded by K // 2 (index -i reads i, H - 1 + i reads H - 1 - i), one accumulator per
output, the K * K taps visited with dy outer and dx inner, both ascending, ``acc = acc + kern[dy][dx] * xpad[i + dy][j + dx]`` in float64.
The product of two fp32 values is exact in float64, so each step rounds once, as the kernel's fused multiply-add does; rounding the result
to fp32 gives the kernel's bits.

``filter2d``: (B, C, H, W) fp32 and (B or 1, K, K) fp32 -> (B, C, H, W) float64, unrounded.  ``usm_sharp``: the reference's
``USMSharp.forward`` with the two blurs restated and every element-wise step a single fp32 torch operation on the CPU, as the module
evaluates them on the device."""
import numpy as np
import torch


def _reflect_index(n, r):
    i = np.arange(-r, n + r)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def filter2d(x, kern):
    x, kern = np.asarray(x), np.asarray(kern)
    assert x.dtype == np.float32 and kern.dtype == np.float32 and x.ndim == 4 and kern.ndim == 3
    B, C, H, W = x.shape
    K = kern.shape[-1]
    r = K // 2
    assert kern.shape[0] in (1, B) and kern.shape[1] == K and K % 2 == 1 and r < H and r < W
    xp = x.astype(np.float64)[:, :, _reflect_index(H, r)][:, :, :, _reflect_index(W, r)]
    k = np.broadcast_to(kern.astype(np.float64), (B, K, K))
    acc = np.zeros((B, C, H, W), dtype=np.float64)
    for dy in range(K):
        for dx in range(K):
            acc = acc + k[:, dy, dx][:, None, None, None] * xp[:, :, dy:dy + H, dx:dx + W]
    return acc


def filter2d_f32(x, kern):
    """the restatement rounded once to fp32, as a torch tensor: what the kernel returns"""
    return torch.from_numpy(filter2d(x, kern).astype(np.float32))


def usm_sharp(img, kern, weight=0.5, threshold=10):
    """img (B, C, H, W) fp32 tensor on the CPU, kern (1, K, K) fp32 tensor"""
    def blur(t):
        return filter2d_f32(t.numpy(), kern.numpy())

    residual = img - blur(img)
    mask = (torch.abs(residual) * 255 > threshold).float()
    soft = blur(mask)
    sharp = torch.clip(img + weight * residual, 0, 1)
    return soft * sharp + (1 - soft) * img
