// Window geometry of the SwinIR attention kernels (swin.hip fp32, swin_bf16.hip bf16): the cyclic shift (torch.roll by -shift), window
// partition, window reverse and the inverse roll are one address map -- token t = i * ws + j of window (wy, wx) of image b is pixel
// ((wy*ws + i + shift) mod H, (wx*ws + j + shift) mod W), read from and written back to that pixel's NHWC row.
#pragma once
#include "dcpt_common.h"

namespace {

constexpr int WT = 64;                 // max tokens per window (ws^2 <= 64)

struct WinGeom {
    int B, H, W, C, heads, hd, ws, shift, nwy, nwx, N, NP;
};

__device__ __forceinline__ int64_t win_token_row(const WinGeom& g, int win, int t) {
    const int per_img = g.nwy * g.nwx;
    const int b = win / per_img, r = win - b * per_img;
    const int wy = r / g.nwx, wx = r - wy * g.nwx;
    const int i = t / g.ws, j = t - i * g.ws;
    int py = wy * g.ws + i + g.shift;
    int px = wx * g.ws + j + g.shift;
    if (py >= g.H) py -= g.H;
    if (px >= g.W) px -= g.W;
    return ((int64_t)b * g.H + py) * g.W + px;
}

inline WinGeom win_geom(int B, int H, int W, int C, int heads, int window, int shift) {
    WinGeom g;
    g.B = B; g.H = H; g.W = W; g.C = C; g.heads = heads; g.hd = C / heads; g.ws = window; g.shift = shift;
    g.nwy = H / window; g.nwx = W / window; g.N = window * window; g.NP = g.N <= 32 ? 32 : 64;
    return g;
}

}  // namespace
