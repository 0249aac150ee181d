// The front end the metric kernels share (metrics.hip: PSNR / SSIM; metrics_ms.hip: MS-SSIM, MATLAB SSIM, the NRMSE range): the value a
// metric is evaluated on, as basicsr/metrics/__init__.py::_images / _to_y forms it.  The window passes and the taps are window_f64.h's, the
// block sum block_sum.h's.  As there, a function whose products feed sums says `#pragma clang fp contract(off)` in its own body: the
// rounding does not depend on where this header is included.
#pragma once
#include <math.h>

#include "dcpt_common.h"
#include "window_f64.h"

namespace {
struct MetricGeom {
    int C, Cp;           // input channels, scored channels (1 for luma)
    int H, W, crop;
    int Hc, Wc;          // cropped size
    int nty, ntx;        // tiles of map positions
    int luma, quant, ssim, int_sse;
    float range;         // 255 or 1
    double c1, c2;
};

// the value the metric is evaluated on, as the host forms it (basicsr/metrics/__init__.py::_images / _to_y)
__device__ __forceinline__ float quantise(float v) { return fminf(fmaxf(rintf(v * 255.0f), 0.0f), 255.0f); }

__device__ __forceinline__ float metric_value(const float* __restrict__ img, int64_t plane, int64_t off, const MetricGeom& m) {
#pragma clang fp contract(off)
    if (!m.luma) {
        const float v = img[off];
        return m.quant ? quantise(v) : v;
    }
    float r = img[off], g = img[off + plane], b = img[off + 2 * plane];
    if (m.quant) {
        r = quantise(r);
        g = quantise(g);
        b = quantise(b);
    }
    // x = value / image_range in fp32, the dot product and (.. + 16) / 255 in fp64, rounded to fp32, times image_range in fp32
    const double xb = (double)__fdiv_rn(b, m.range), xg = (double)__fdiv_rn(g, m.range), xr = (double)__fdiv_rn(r, m.range);
    const double y = (xb * 24.966 + xg * 128.553 + xr * 65.481 + 16.0) / 255.0;
    return __fmul_rn((float)y, m.range);
}

// the geometry and constants every metric launcher fills the same way (tiles are set by the caller)
inline MetricGeom metric_geom(int C, int H, int W, int crop, int luma, int range) {
    MetricGeom m{};
    m.C = C;
    m.luma = luma && C == 3;
    m.Cp = m.luma ? 1 : C;
    m.H = H; m.W = W; m.crop = crop;
    m.Hc = H - 2 * crop; m.Wc = W - 2 * crop;
    m.quant = range == 255;
    m.int_sse = m.quant && !m.luma;
    m.range = (float)range;
    m.c1 = (0.01 * range) * (0.01 * range);
    m.c2 = (0.03 * range) * (0.03 * range);
    return m;
}
}  // namespace
