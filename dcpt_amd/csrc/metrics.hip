// Validation metrics on the device: the sums behind PSNR and SSIM of a batch of NCHW image pairs (include/dcpt_hip.h dcpt_imgmetric),
// the arithmetic of basicsr/metrics (_images, _to_y, _ssim) step by step: quantise to 0..255 with round-half-even, crop by addressing,
// optional BT.601 luma, squared error per image, and the 11-tap Gaussian "valid" SSIM map per (image, channel) in fp64.
//
// One workgroup per TH x TW tile of SSIM-map positions of one (image, channel).  It stages the (TH + 10) x (TW + 10) values of both
// images in LDS (every value on every path is an fp32 number: an integer 0..255, an fp32 luma, or the fp32 input itself), runs the
// horizontal pass of x, y, x^2, y^2, xy into LDS in fp64, then the vertical pass and the SSIM value in registers (both passes and the taps:
// window_f64.h; the front end: metric_front.h; the block sum: block_sum.h).  The squared error is taken while staging, each pixel by the one
// tile that owns it.  Every workgroup stores one SSIM partial and one squared-error partial with ordinary stores; a second kernel adds the
// partials of an image in a fixed order.  No atomics: two runs give identical bits.
#include <math.h>

#include "kernels.h"
#include "metric_front.h"
#include "prof.h"

// every product and sum rounds on its own, as numpy's element-wise passes do (the shared headers say so per function; this covers the rest)
#pragma clang fp contract(off)

namespace {
constexpr int TH = METRIC_TH, TW = METRIC_TW, WIN = METRIC_WIN;
constexpr int SH = METRIC_SH, SW = METRIC_SW;   // staged rows / columns
constexpr int NT = METRIC_NT;

__global__ __launch_bounds__(NT) void metric_tile_kernel(const float* __restrict__ img, const float* __restrict__ img2,
                                                         double* __restrict__ ssim_part, unsigned long long* __restrict__ sse_part,
                                                         MetricGeom m, Gauss gw) {
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
    const bool last_y = ty == m.nty - 1, last_x = tx == m.ntx - 1;

    // ---- stage + squared error ----
    unsigned long long sse_i = 0;
    double sse_f = 0.0;
    for (int i = tid; i < SH * SW; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 + r, gx = x0 + c;
        float vx = 0.f, vy = 0.f;
        if (gy < m.Hc && gx < m.Wc) {
            const int64_t off = (int64_t)(gy + m.crop) * m.W + (gx + m.crop);
            vx = metric_value(px, plane, off, m);
            vy = metric_value(py, plane, off, m);
            if ((r < TH || last_y) && (c < TW || last_x)) {   // the halo belongs to the next tile, except behind the last one
                if (m.int_sse) {
                    const int d = (int)vx - (int)vy;
                    sse_i += (unsigned long long)(d * d);
                } else {
                    const double d = (double)vx - (double)vy;
                    sse_f += d * d;
                }
            }
        }
        sx[r][c] = vx;
        sy[r][c] = vy;
    }
    __syncthreads();

    double acc = 0.0;
    if (m.ssim) {
        const Gauss taps = gw;   // (a copy made here: the PSNR-only path never loads the taps; window_f64.h)
        gauss_rows<float, SW>(sx, sy, hp, taps);
        __syncthreads();
        for (int i = tid; i < TH * TW; i += NT) {
            const int r = i / TW, c = i - r * TW;
            if (y0 + r >= m.Hc - (WIN - 1) || x0 + c >= m.Wc - (WIN - 1)) continue;
            const Moments o = gauss_col(hp, r, c, taps);
            const double cs = (2.0 * o.s12 + m.c2) / (o.s1 + o.s2 + m.c2);
            acc += ((2.0 * o.mu12 + m.c1) / (o.mu1_sq + o.mu2_sq + m.c1)) * cs;
        }
        acc = block_sum(acc, red);
    }
    unsigned long long sse_bits;
    if (m.int_sse) {
        sse_bits = block_sum(sse_i, reinterpret_cast<unsigned long long*>(red));
    } else {
        sse_bits = (unsigned long long)__double_as_longlong(block_sum(sse_f, red));
    }
    if (tid == 0) {
        const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        ssim_part[slot] = acc;
        sse_part[slot] = sse_bits;
    }
}

// one workgroup per image: ssim_out[b][c] = sum over the tiles of (b, c); sse_out[b] = sum over the tiles of every channel of b
__global__ __launch_bounds__(NT) void metric_reduce_kernel(const double* __restrict__ ssim_part, const unsigned long long* __restrict__ sse_part,
                                                           double* __restrict__ ssim_out, unsigned long long* __restrict__ sse_out, int Cp,
                                                           int ntiles, int ssim, int int_sse) {
    __shared__ double red[NT];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (ssim) {
        for (int c = 0; c < Cp; ++c) {
            const double* p = ssim_part + ((int64_t)b * Cp + c) * ntiles;
            double a = 0.0;
            for (int i = tid; i < ntiles; i += NT) a += p[i];
            a = block_sum(a, red);
            if (tid == 0) ssim_out[(int64_t)b * Cp + c] = a;
        }
    }
    const unsigned long long* q = sse_part + (int64_t)b * Cp * ntiles;
    const int n = Cp * ntiles;
    if (int_sse) {
        unsigned long long a = 0;
        for (int i = tid; i < n; i += NT) a += q[i];
        a = block_sum(a, reinterpret_cast<unsigned long long*>(red));
        if (tid == 0) sse_out[b] = a;
    } else {
        double a = 0.0;
        for (int i = tid; i < n; i += NT) a += __longlong_as_double((long long)q[i]);
        a = block_sum(a, red);
        if (tid == 0) sse_out[b] = (unsigned long long)__double_as_longlong(a);
    }
}
}  // namespace

int metric_num_tiles(int Hc, int Wc) {
    const int oh = Hc > WIN - 1 ? Hc - (WIN - 1) : 1, ow = Wc > WIN - 1 ? Wc - (WIN - 1) : 1;   // (PSNR alone may see an image under 11 pixels)
    return cdiv(oh, TH) * cdiv(ow, TW);
}

int launch_imgmetric(const float* img, const float* img2, void* sse_out, double* ssim_out, double* ssim_part, void* sse_part, int B, int C,
                     int H, int W, int crop, int luma, int range, int want_ssim, hipStream_t s) {
    MetricGeom m = metric_geom(C, H, W, crop, luma, range);
    const int oh = m.Hc > WIN - 1 ? m.Hc - (WIN - 1) : 1, ow = m.Wc > WIN - 1 ? m.Wc - (WIN - 1) : 1;
    m.nty = cdiv(oh, TH); m.ntx = cdiv(ow, TW);
    m.ssim = want_ssim;
    const Gauss gw = gauss_taps();
    const int ntiles = m.nty * m.ntx;
    trace_tag(want_ssim ? "metric.tile_ssim" : "metric.tile_psnr");
    metric_tile_kernel<<<dim3((unsigned)ntiles, (unsigned)(B * m.Cp)), dim3(NT), 0, s>>>(img, img2, ssim_part, (unsigned long long*)sse_part, m,
                                                                                       gw);
    DCPT_CHECK_LAUNCH("imgmetric tile");
    trace_tag("metric.reduce");
    metric_reduce_kernel<<<dim3((unsigned)B), dim3(NT), 0, s>>>(ssim_part, (const unsigned long long*)sse_part, ssim_out,
                                                                (unsigned long long*)sse_out, m.Cp, ntiles, want_ssim, m.int_sse);
    DCPT_CHECK_LAUNCH("imgmetric reduce");
    return DCPT_OK;
}
