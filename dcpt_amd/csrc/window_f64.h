// The fp64 window arithmetic the SSIM kernels share (metrics.hip, metrics_ms.hip, ssim_loss.hip): the 11 Gaussian taps and the separable
// pass of the five maps x, y, x^2, y^2, xy over one METRIC_TH x METRIC_TW tile -- rows into LDS, then columns and the moments every SSIM form
// is built from.  Every product and sum rounds on its own, as numpy's element-wise passes do (mu1 * mu1 is one array there, the subtraction
// another): each function whose products feed sums says `#pragma clang fp contract(off)` in its own body, so the rounding depends neither
// on where this header is included nor on the including file's setting, and it leaves that setting alone.
#pragma once
#include <math.h>

#include "block_sum.h"
#include "kernels.h"

namespace {
constexpr int METRIC_WIN = 11;
constexpr int METRIC_NT = BLOCK_NT;                                // threads per workgroup of every window kernel
constexpr int METRIC_SH = METRIC_TH + METRIC_WIN - 1;              // rows the two passes read for one tile
constexpr int METRIC_SW = METRIC_TW + METRIC_WIN - 1;              // columns

struct Gauss {
    double g[METRIC_WIN];
};

// cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 sigma^2)), normalised to sum 1
inline Gauss gauss_taps() {
    Gauss gw;
    double sum = 0.0;
    for (int i = 0; i < METRIC_WIN; ++i) {
        const double x = (double)i - 5.0;
        gw.g[i] = exp(-(x * x) / (2.0 * 1.5 * 1.5));
        sum += gw.g[i];
    }
    for (int i = 0; i < METRIC_WIN; ++i) gw.g[i] /= sum;
    return gw;
}

// The taps are a kernel argument, and where the compiler loads them follows from what the caller hands in.  A kernel that always runs the
// passes (msssim_level_kernel, ssim_matlab_tile_kernel) hands in the argument itself: the loads sit at the kernel's entry, under the staging
// loads.  A kernel that can skip the passes (metric_tile_kernel without SSIM) or that had them written out in its body (ssim_tile_kernel)
// hands in a local copy made where the passes start: the loads sit there, and the path around them keeps the instructions it had.
//
// horizontal pass of x, y, x^2, y^2, xy over the staged rows (elements of type T, LD per row): hp[j][r][c] = sum_k g[k] v_j[r][c + k]
template <typename T, int LD>
__device__ __forceinline__ void gauss_rows(const T (*sx)[LD], const T (*sy)[LD], double (*hp)[METRIC_SH][METRIC_TW], const Gauss& gw) {
#pragma clang fp contract(off)
    for (int i = threadIdx.x; i < METRIC_SH * METRIC_TW; i += METRIC_NT) {
        const int r = i / METRIC_TW, c = i - r * METRIC_TW;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
        for (int k = 0; k < METRIC_WIN; ++k) {
            const double x = (double)sx[r][c + k], y = (double)sy[r][c + k], g = gw.g[k];
            a0 += g * x;
            a1 += g * y;
            a2 += g * (x * x);
            a3 += g * (y * y);
            a4 += g * (x * y);
        }
        hp[0][r][c] = a0;
        hp[1][r][c] = a1;
        hp[2][r][c] = a2;
        hp[3][r][c] = a3;
        hp[4][r][c] = a4;
    }
}

struct Moments {
    double mu1, mu2, mu1_sq, mu2_sq, mu12, s1, s2, s12;
};

// vertical pass at (r, c): the means, their products and the (co)variances
__device__ __forceinline__ Moments gauss_col(const double (*hp)[METRIC_SH][METRIC_TW], int r, int c, const Gauss& gw) {
#pragma clang fp contract(off)
    double mu1 = 0.0, mu2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int k = 0; k < METRIC_WIN; ++k) {
        const double g = gw.g[k];
        mu1 += g * hp[0][r + k][c];
        mu2 += g * hp[1][r + k][c];
        e11 += g * hp[2][r + k][c];
        e22 += g * hp[3][r + k][c];
        e12 += g * hp[4][r + k][c];
    }
    Moments o;
    o.mu1 = mu1;
    o.mu2 = mu2;
    o.mu1_sq = mu1 * mu1;
    o.mu2_sq = mu2 * mu2;
    o.mu12 = mu1 * mu2;
    o.s1 = e11 - o.mu1_sq;
    o.s2 = e22 - o.mu2_sq;
    o.s12 = e12 - o.mu12;
    return o;
}
}  // namespace
