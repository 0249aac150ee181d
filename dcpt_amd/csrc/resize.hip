// The resize of the second-order degradation chain (include/dcpt_hip.h dcpt_interp_fwd): F.interpolate's `area`, `bilinear` and `bicubic`
// modes (align_corners=False, no antialiasing) on dense NCHW fp32 planes; ONE launch, no workspace, no atomics, the same bits on every run.
//
// Arithmetic, per output (i, j), all in fp64 (the header states the taps of an axis):
//     acc = 0;  for a ascending:  { inner = 0;  for b ascending: inner = fma(ww[b], (double)x[ia][jb], inner);  acc = fma(wh[a], inner, acc); }
//     y = (float)acc, the one fp32 rounding (after the optional clamp and 8-bit rounding).
//
// One workgroup of 256 owns a 16 x 64 output tile of an image and walks the image's C channels (and, past 65535 images, further images)
// with it.  The taps of the tile's 16 rows and 64 columns -- first index, count, up to four fp64 weights -- are computed ONCE per
// workgroup by its first 80 lanes and kept in LDS (3.2 KB); a lane takes its column's taps into registers and reads its rows' taps as
// wave-wide broadcasts.  A wave owns one tile row at a time (lane = column, four rows per lane), so a wave's source reads of one tap run
// along a source row and its store is one 256-byte row segment.
//
// The source is NOT staged in LDS: it is read through the vector caches.  At the chain's strongest reduction (ratio 6.7 per axis) the
// footprint of an area tile is about 108 x 428 source pixels, which as fp32 (185 KB) does not fit the 160 KB of LDS at this tile; a tile
// sized by the ratio would shrink to a few rows and lose the row-segment stores.  Every source line a wave touches is used in full by that
// wave (its lanes' tap runs are adjacent) within a few iterations, so the re-reads hit the CU's L1.
#include <math.h>
#include <stdint.h>

#include "kernels.h"
#include "prof.h"

namespace {
constexpr int NT = 256;
constexpr int TW = 64, TH = 16;              // the output tile
constexpr int ROWS = TH / (NT / 64);         // tile rows per lane: rows wave, wave + 4, ..
constexpr int MODE_AREA = 0, MODE_BILINEAR = 1, MODE_BICUBIC = 2;   // include/dcpt_hip.h DCPT_INTERP_*
constexpr int F_CLIP = 1, F_ROUND8 = 2;
constexpr int MAX_GY = 65535;

struct InterpGeom {
    int B, C, H, W, Ho, Wo;
    int gx;            // tiles per row of tiles
    int flags;
    double rh, rw;     // source pixels per destination pixel
};

// the taps of output index d of an axis (n source, m destination samples, ratio r): source indices clamp(first + k, 0, n - 1) for
// k = 0 .. cnt - 1 with the weights w[k]; an area tap run needs no clamp and every tap weighs w[0]
template <int MODE>
__device__ __forceinline__ void axis_taps(int d, int n, int m, double r, int& first, int& cnt, double (&w)[4]) {
#pragma clang fp contract(off)   // the source coordinate as the header writes it: a product, then a difference
    w[0] = w[1] = w[2] = w[3] = 0.0;
    if (MODE == MODE_AREA) {
        const int64_t s = (int64_t)d * n / m, e = ((int64_t)(d + 1) * n + m - 1) / m;
        first = (int)s;
        cnt = (int)(e - s);
        w[0] = 1.0 / (double)cnt;
    } else if (MODE == MODE_BILINEAR) {
        const double src = fmax(((double)d + 0.5) * r - 0.5, 0.0);
        const double f = fmin(floor(src), (double)(n - 1));
        const double t = src - f;
        first = (int)f;
        cnt = 2;
        w[0] = 1.0 - t;
        w[1] = t;
    } else {
        constexpr double A = -0.75;
        const double src = ((double)d + 0.5) * r - 0.5;
        const double f = floor(src);
        const double t = src - f;
        first = (int)fmin(fmax(f, -2.0), (double)n + 1.0) - 1;   // (beyond that every clamped index is the edge sample anyway)
        cnt = 4;
        const double xs[4] = {t + 1.0, t, 1.0 - t, 2.0 - t};
        w[0] = ((A * xs[0] - 5.0 * A) * xs[0] + 8.0 * A) * xs[0] - 4.0 * A;
        w[1] = ((A + 2.0) * xs[1] - (A + 3.0)) * xs[1] * xs[1] + 1.0;
        w[2] = ((A + 2.0) * xs[2] - (A + 3.0)) * xs[2] * xs[2] + 1.0;
        w[3] = ((A * xs[3] - 5.0 * A) * xs[3] + 8.0 * A) * xs[3] - 4.0 * A;
    }
}

__device__ __forceinline__ float finish(double v, int flags) {
    if (flags & F_CLIP) v = fmin(fmax(v, 0.0), 1.0);
    if (flags & F_ROUND8) v = rint(255.0 * v) / 255.0;
    return (float)v;
}

template <int MODE>
__global__ __launch_bounds__(NT) void interp_kernel(const float* __restrict__ x, float* __restrict__ y, InterpGeom m) {
    __shared__ int s_first[TH + TW], s_cnt[TH + TW];   // rows 0 .. TH - 1, then columns
    __shared__ double s_w[TH + TW][4];
    const int ty0 = blockIdx.x / m.gx, tx0 = blockIdx.x - ty0 * m.gx;
    const int y0 = ty0 * TH, x0 = tx0 * TW;
    if (threadIdx.x < TH + TW) {
        const bool row = threadIdx.x < TH;
        const int d = row ? y0 + threadIdx.x : x0 + threadIdx.x - TH;
        const int n = row ? m.H : m.W, mm = row ? m.Ho : m.Wo;
        int first = 0, cnt = 0;
        double w[4] = {0.0, 0.0, 0.0, 0.0};
        if (d < mm) axis_taps<MODE>(d, n, mm, row ? m.rh : m.rw, first, cnt, w);
        s_first[threadIdx.x] = first;
        s_cnt[threadIdx.x] = cnt;
#pragma unroll
        for (int k = 0; k < 4; ++k) s_w[threadIdx.x][k] = w[k];
    }
    __syncthreads();

    const int tx = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ox = x0 + tx;
    if (ox >= m.Wo) return;   // (after the only barrier)
    const int fw = s_first[TH + tx], cw = s_cnt[TH + tx];
    double ww[4];
    int jb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ww[k] = s_w[TH + tx][k];
        jb[k] = min(max(fw + k, 0), m.W - 1);
    }
    constexpr int KT = MODE == MODE_BILINEAR ? 2 : 4;
    const int64_t plane_in = (int64_t)m.H * m.W, plane_out = (int64_t)m.Ho * m.Wo;
    for (int b = blockIdx.y; b < m.B; b += gridDim.y) {
        for (int c = 0; c < m.C; ++c) {
            const float* xp = x + ((int64_t)b * m.C + c) * plane_in;
            float* yp = y + ((int64_t)b * m.C + c) * plane_out;
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const int row = wave + i * (NT / 64), oy = y0 + row;
                if (oy >= m.Ho) break;
                const int fh = s_first[row], ch = s_cnt[row];
                double acc = 0.0;
                if (MODE == MODE_AREA) {
                    const double wh = s_w[row][0];
                    const float* xr = xp + (int64_t)fh * m.W + fw;   // s .. e - 1 lie inside the plane on both axes
                    for (int a = 0; a < ch; ++a, xr += m.W) {
                        double inner = 0.0;
                        for (int k = 0; k < cw; ++k) inner = fma(ww[0], (double)xr[k], inner);
                        acc = fma(wh, inner, acc);
                    }
                } else {
#pragma unroll
                    for (int a = 0; a < KT; ++a) {
                        const float* xr = xp + (int64_t)min(max(fh + a, 0), m.H - 1) * m.W;
                        double inner = 0.0;
#pragma unroll
                        for (int k = 0; k < KT; ++k) inner = fma(ww[k], (double)xr[jb[k]], inner);
                        acc = fma(s_w[row][a], inner, acc);
                    }
                }
                yp[(int64_t)oy * m.Wo + ox] = finish(acc, m.flags);
            }
        }
    }
}
}  // namespace

int launch_interp_fwd(const float* x, float* y, int B, int C, int H, int W, int Ho, int Wo, int mode, double ratio_h, double ratio_w, int flags,
                      hipStream_t s) {
    InterpGeom m{};
    m.B = B; m.C = C; m.H = H; m.W = W; m.Ho = Ho; m.Wo = Wo;
    m.gx = cdiv(Wo, TW);
    m.flags = flags;
    m.rh = ratio_h; m.rw = ratio_w;
    const dim3 grid((unsigned)(m.gx * cdiv(Ho, TH)), (unsigned)(B < MAX_GY ? B : MAX_GY)), block(NT);   // (a plane of at most 2^30 pixels: < 2^27 tiles)
    trace_tag("degrade.interp");
    if (mode == MODE_AREA) interp_kernel<MODE_AREA><<<grid, block, 0, s>>>(x, y, m);
    else if (mode == MODE_BILINEAR) interp_kernel<MODE_BILINEAR><<<grid, block, 0, s>>>(x, y, m);
    else interp_kernel<MODE_BICUBIC><<<grid, block, 0, s>>>(x, y, m);
    DCPT_CHECK_LAUNCH("interp_fwd");
    return DCPT_OK;
}
