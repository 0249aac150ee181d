// The remaining reference metrics on the device (include/dcpt_hip.h dcpt_msssim, dcpt_ssim_matlab, dcpt_imgrange): the sums behind
// basicsr/metrics calculate_msssim, calculate_ssim_matlab and the value range calculate_nrmse divides by, step by step as the host forms
// compute them.  The front end (quantise, crop by addressing, BT.601 luma) is metrics.hip's own (metric_front.h), the Gaussian taps and
// the two window passes are window_f64.h's, the block tree and the reduce kernel block_sum.h's.  All window arithmetic is fp64; every
// product and sum rounds on its own.
//
// MS-SSIM, all levels in ONE launch.  The reference does not decimate: evaluation k scores channel k mod C' of the images after k passes of
// the 2 x 2 box filter anchored at (0, 0), out[y][x] = 0.25 ((a[y][x] + a[y][x+1]) + (a[y+1][x] + a[y+1][x+1])), an index past the last row
// or column reading the last one.  The grid is (tile, image x level).  The workgroup of level k stages the (TH + 10 + k) x (TW + 10 + k)
// metric values of its tile in fp64 with indices clamped to the cropped image's last row / column, then applies the k box passes in LDS in
// order; each pass shrinks the valid region by one row and one column.  Clamped staging plus in-order passes gives exactly the sequentially
// blurred image: if t[i] holds the p-times blurred value at index min(g0 + i, n - 1), then 0.25 ((t[i] + t[i+1]) + ..) is the (p + 1)-times
// blurred value at min(g0 + i, n - 1), because past the edge all four terms are the same number v and 0.25 ((v + v) + (v + v)) = v exactly.
// A pass reads the values of its elements into registers, synchronises, and writes them back (no second buffer).  The two Gaussian passes
// and the SSIM / CS values follow as in metrics.hip.
// LDS budget (static, 64 KB limit): fp64 staging 2 x 33 x 49 x 8 = 25 872 B at the deepest level (k = 7) + the horizontal-pass buffer
// 5 x 26 x 32 x 8 = 33 280 B + the reduction's 2 048 B = 61 200 B.  Rows of 32 / 49 consecutive doubles: a wave's ds_read_b64 of one row
// segment is conflict-free (32 lanes x 8 B = the 64 banks once).
//
// MATLAB SSIM: the same five windowed moments at EVERY pixel under replicate padding of 5; the tile covers output pixels, its halo of 5 on
// all sides is staged with clamped indices.  fp32 staging (every metric value is an fp32 number), as metrics.hip.
//
// Range: per-image min and max of the first image's metric values over all scored channels (exact, so the order is immaterial).
//
// Every workgroup stores its partials with ordinary stores; a second kernel (sum_reduce_kernel of block_sum.h, or the range's own) adds or
// min / max-es them in a fixed order.  No atomics.
#include <math.h>

#include "kernels.h"
#include "metric_front.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {
constexpr int TH = METRIC_TH, TW = METRIC_TW, WIN = METRIC_WIN, PAD = WIN / 2;
constexpr int SH = METRIC_SH, SW = METRIC_SW;         // rows / columns the Gaussian passes read
constexpr int NT = METRIC_NT;
constexpr int KMAX = MSSSIM_MAX_LEVELS - 1;           // box passes of the deepest level
constexpr int BH = SH + KMAX, BW = SW + KMAX;         // staged rows / columns of the deepest level
constexpr int BPT = (BH * BW + NT - 1) / NT;          // elements of one box pass per thread
static_assert(2 * BH * BW * 8 + 5 * SH * TW * 8 + NT * 8 <= 64 * 1024, "static LDS of the MS-SSIM kernel");

// ---- MS-SSIM: grid (tile, image * L + level) -> part[image][level][tile][2] = sums of the SSIM map and of the CS map -------------------
__global__ __launch_bounds__(NT) void msssim_level_kernel(const float* __restrict__ img, const float* __restrict__ img2, double* __restrict__ part,
                                                          MetricGeom m, Gauss gw, int L) {
    __shared__ double sx[BH][BW], sy[BH][BW];
    __shared__ double hp[5][SH][TW];
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / m.ntx, tx = blockIdx.x - ty * m.ntx;
    const int b = blockIdx.y / L, k = blockIdx.y - b * L;
    const int ch = k % m.Cp;   // the reference's blur sits inside its channel loop: evaluation k sees channel k mod C' after k blurs
    const int64_t plane = (int64_t)m.H * m.W;
    const float* px = img + ((int64_t)b * m.C + ch) * plane;
    const float* py = img2 + ((int64_t)b * m.C + ch) * plane;
    const int y0 = ty * TH, x0 = tx * TW;

    // ---- stage, indices clamped to the cropped image ----
    const int rows = SH + k, cols = SW + k;
    for (int i = tid; i < rows * cols; i += NT) {
        const int r = i / cols, c = i - r * cols;
        const int gy = min(y0 + r, m.Hc - 1), gx = min(x0 + c, m.Wc - 1);
        const int64_t off = (int64_t)(gy + m.crop) * m.W + (gx + m.crop);
        sx[r][c] = (double)metric_value(px, plane, off, m);
        sy[r][c] = (double)metric_value(py, plane, off, m);
    }
    __syncthreads();

    // ---- k box passes, in place through registers ----
    for (int p = 1; p <= k; ++p) {
        const int nr = rows - p, nc = cols - p;
        double vx[BPT], vy[BPT];
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int i = tid + e * NT;
            if (i < nr * nc) {
                const int r = i / nc, c = i - r * nc;
                vx[e] = 0.25 * ((sx[r][c] + sx[r][c + 1]) + (sx[r + 1][c] + sx[r + 1][c + 1]));
                vy[e] = 0.25 * ((sy[r][c] + sy[r][c + 1]) + (sy[r + 1][c] + sy[r + 1][c + 1]));
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int i = tid + e * NT;
            if (i < nr * nc) {
                const int r = i / nc, c = i - r * nc;
                sx[r][c] = vx[e];
                sy[r][c] = vy[e];
            }
        }
        __syncthreads();
    }

    gauss_rows<double, BW>(sx, sy, hp, gw);
    __syncthreads();
    double acc_ssim = 0.0, acc_cs = 0.0;
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        if (y0 + r >= m.Hc - (WIN - 1) || x0 + c >= m.Wc - (WIN - 1)) continue;
        const Moments o = gauss_col(hp, r, c, gw);
        const double cs = (2.0 * o.s12 + m.c2) / (o.s1 + o.s2 + m.c2);
        acc_ssim += ((2.0 * o.mu12 + m.c1) / (o.mu1_sq + o.mu2_sq + m.c1)) * cs;
        acc_cs += cs;
    }
    acc_ssim = block_sum(acc_ssim, red);
    acc_cs = block_sum(acc_cs, red);
    if (tid == 0) {
        const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[2 * slot] = acc_ssim;
        part[2 * slot + 1] = acc_cs;
    }
}

// ---- MATLAB SSIM: grid (tile of output pixels, image * C' + channel) -> part[image][channel][tile] ------------------------------------
__global__ __launch_bounds__(NT) void ssim_matlab_tile_kernel(const float* __restrict__ img, const float* __restrict__ img2,
                                                              double* __restrict__ part, MetricGeom m, Gauss gw) {
    __shared__ float sx[SH][SW], sy[SH][SW];
    __shared__ double hp[5][SH][TW];
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / m.ntx, tx = blockIdx.x - ty * m.ntx;
    const int b = blockIdx.y / m.Cp, ch = blockIdx.y - b * m.Cp;
    const int64_t plane = (int64_t)m.H * m.W;
    const float* px = img + ((int64_t)b * m.C + ch) * plane;
    const float* py = img2 + ((int64_t)b * m.C + ch) * plane;
    const int y0 = ty * TH, x0 = tx * TW;

    // ---- stage the tile and its halo of 5, replicate addressing ----
    for (int i = tid; i < SH * SW; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int gy = min(max(y0 + r - PAD, 0), m.Hc - 1), gx = min(max(x0 + c - PAD, 0), m.Wc - 1);
        const int64_t off = (int64_t)(gy + m.crop) * m.W + (gx + m.crop);
        sx[r][c] = metric_value(px, plane, off, m);
        sy[r][c] = metric_value(py, plane, off, m);
    }
    __syncthreads();
    gauss_rows<float, SW>(sx, sy, hp, gw);
    __syncthreads();
    double acc = 0.0;
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        if (y0 + r >= m.Hc || x0 + c >= m.Wc) continue;
        const Moments o = gauss_col(hp, r, c, gw);
        // the reference's SSIM_MATLAB_Pytorch._ssim: one quotient of two products
        acc += ((2.0 * o.mu12 + m.c1) * (2.0 * o.s12 + m.c2)) / ((o.mu1_sq + o.mu2_sq + m.c1) * (o.s1 + o.s2 + m.c2));
    }
    acc = block_sum(acc, red);
    if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// ---- range: grid (chunk of RANGE_CHUNK scored values, image) -> part[image][chunk][2] = min, max ---------------------------------------
struct MinMax {
    float lo, hi;
};

__device__ __forceinline__ void block_minmax(float& lo, float& hi, MinMax* red) {   // (the tree of block_sum.h; exact, so any order would do)
    const MinMax r = block_tree(MinMax{lo, hi}, red, [](MinMax a, MinMax b) { return MinMax{fminf(a.lo, b.lo), fmaxf(a.hi, b.hi)}; });
    lo = r.lo;
    hi = r.hi;
}

__global__ __launch_bounds__(NT) void range_tile_kernel(const float* __restrict__ img, double* __restrict__ part, MetricGeom m) {
    __shared__ MinMax red[NT];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t plane = (int64_t)m.H * m.W, cplane = (int64_t)m.Hc * m.Wc, n = cplane * m.Cp;
    const float* pb = img + (int64_t)b * m.C * plane;
    float lo = INFINITY, hi = -INFINITY;
    const int64_t base = (int64_t)blockIdx.x * METRIC_RANGE_CHUNK;
    for (int i = tid; i < METRIC_RANGE_CHUNK; i += NT) {
        const int64_t idx = base + i;
        if (idx >= n) break;
        const int ch = (int)(idx / cplane);
        const int64_t rem = idx - (int64_t)ch * cplane;
        const int y = (int)(rem / m.Wc), x = (int)(rem - (int64_t)y * m.Wc);
        const float v = metric_value(pb + (int64_t)ch * plane, plane, (int64_t)(y + m.crop) * m.W + (x + m.crop), m);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax(lo, hi, red);
    if (tid == 0) {
        const int64_t slot = (int64_t)b * gridDim.x + blockIdx.x;
        part[2 * slot] = (double)lo;
        part[2 * slot + 1] = (double)hi;
    }
}

__global__ __launch_bounds__(NT) void range_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int nchunks) {
    __shared__ MinMax red[NT];
    const int tid = threadIdx.x, b = blockIdx.x;
    const double* p = part + (int64_t)b * nchunks * 2;
    float lo = INFINITY, hi = -INFINITY;   // (the partials are fp32 numbers)
    for (int i = tid; i < nchunks; i += NT) {
        lo = fminf(lo, (float)p[2 * i]);
        hi = fmaxf(hi, (float)p[2 * i + 1]);
    }
    block_minmax(lo, hi, red);
    if (tid == 0) {
        out[2 * b] = (double)lo;
        out[2 * b + 1] = (double)hi;
    }
}
}  // namespace

int ssim_matlab_num_tiles(int Hc, int Wc) { return cdiv(Hc, TH) * cdiv(Wc, TW); }

int64_t imgrange_num_chunks(int Cp, int Hc, int Wc) { return cdiv64((int64_t)Cp * Hc * Wc, METRIC_RANGE_CHUNK); }

int launch_msssim(const float* img, const float* img2, double* out, double* part, int B, int C, int H, int W, int crop, int luma, int range,
                  int levels, hipStream_t s) {
    MetricGeom m = metric_geom(C, H, W, crop, luma, range);
    m.nty = cdiv(m.Hc - (WIN - 1), TH);
    m.ntx = cdiv(m.Wc - (WIN - 1), TW);
    const Gauss gw = gauss_taps();
    const int ntiles = m.nty * m.ntx;
    trace_tag("metric.ms_level");
    msssim_level_kernel<<<dim3((unsigned)ntiles, (unsigned)(B * levels)), dim3(NT), 0, s>>>(img, img2, part, m, gw, levels);
    DCPT_CHECK_LAUNCH("msssim level");
    trace_tag("metric.ms_reduce");
    sum_reduce_kernel<SUM_PLAIN><<<dim3((unsigned)(B * levels)), dim3(NT), 0, s>>>(part, out, ntiles, 2, 0);
    DCPT_CHECK_LAUNCH("msssim reduce");
    return DCPT_OK;
}

int launch_ssim_matlab(const float* img, const float* img2, double* out, double* part, int B, int C, int H, int W, int crop, int luma, int range,
                       hipStream_t s) {
    MetricGeom m = metric_geom(C, H, W, crop, luma, range);
    m.nty = cdiv(m.Hc, TH);
    m.ntx = cdiv(m.Wc, TW);
    const Gauss gw = gauss_taps();
    const int ntiles = m.nty * m.ntx;
    trace_tag("metric.matlab_tile");
    ssim_matlab_tile_kernel<<<dim3((unsigned)ntiles, (unsigned)(B * m.Cp)), dim3(NT), 0, s>>>(img, img2, part, m, gw);
    DCPT_CHECK_LAUNCH("ssim_matlab tile");
    trace_tag("metric.matlab_reduce");
    sum_reduce_kernel<SUM_PLAIN><<<dim3((unsigned)(B * m.Cp)), dim3(NT), 0, s>>>(part, out, ntiles, 1, 0);
    DCPT_CHECK_LAUNCH("ssim_matlab reduce");
    return DCPT_OK;
}

int launch_imgrange(const float* img, double* out, double* part, int B, int C, int H, int W, int crop, int luma, int range, hipStream_t s) {
    const MetricGeom m = metric_geom(C, H, W, crop, luma, range);
    const int nchunks = (int)imgrange_num_chunks(m.Cp, m.Hc, m.Wc);
    trace_tag("metric.range_tile");
    range_tile_kernel<<<dim3((unsigned)nchunks, (unsigned)B), dim3(NT), 0, s>>>(img, part, m);
    DCPT_CHECK_LAUNCH("imgrange tile");
    trace_tag("metric.range_reduce");
    range_reduce_kernel<<<dim3((unsigned)B), dim3(NT), 0, s>>>(part, out, nchunks);
    DCPT_CHECK_LAUNCH("imgrange reduce");
    return DCPT_OK;
}
