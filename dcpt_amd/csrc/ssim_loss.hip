// SSIM as a training loss on the device (include/dcpt_hip.h dcpt_ssim_loss_fwd / dcpt_ssim_loss_bwd): the per-(image, channel) sums of the
// fp64 SSIM map of two fp32 NCHW images, and the gradient of a weighted sum of those maps with respect to the first image.  The arithmetic
// of the reference's calculate_ssim_pt / _ssim_pth (basicsr/metrics/psnr_ssim.py:436-480, :515-559) without its five grouped fp64
// convolutions: crop by addressing, optional BT.601 luma in fp32, everything after that in fp64.
//
// With g the 11-tap Gaussian, G* the separable "valid" window and, per map position,
//     mx = G*x, my = G*y, sxx = G*(x x) - mx^2, syy = G*(y y) - my^2, sxy = G*(x y) - mx my
//     A1 = 2 mx my + c1, A2 = 2 sxy + c2, B1 = mx^2 + my^2 + c1, B2 = sxx + syy + c2, S = A1 A2 / (B1 B2)
// the gradient of sum_p w S(p) with respect to x is
//     dx(q) = (Gt*Pa)(q) + 2 x(q) (Gt*Pb)(q) + y(q) (Gt*Pc)(q)
//     Pa = w [2 my (A2 - A1) / (B1 B2) - S (2 mx / B1 - 2 mx / B2)],  Pb = -w S / B2,  Pc = 2 w A1 / (B1 B2)
// where Gt* is the transposed ("full") window over maps that are zero outside the valid region.
//
// Forward: one workgroup per TH x TW tile of map positions of one (image, channel), staged as metrics.hip stages it, the two window passes
// and the taps shared with it (window_f64.h); one partial per workgroup, a second kernel (sum_reduce_kernel of block_sum.h) adds an image's
// partials in a fixed order.  Backward: (a) the same tile kernel writes Pa, Pb, Pc as three fp64
// planes of the map's size, (b) a gather kernel, one workgroup per TH x TW tile of INPUT pixels, stages the planes with a 10-wide halo
// (zero outside the map by bounds in the load), runs the transposed separable pass, combines with x and y, applies the luma chain rule and
// rounds once to fp32.  It writes every element of dpred, the zeros of the crop border included.  The batch goes through the planes in
// chunks of whole images.  No atomics anywhere: the same input gives the same bits.
#include <math.h>

#include "kernels.h"
#include "prof.h"
#include "window_f64.h"

// every product and sum rounds on its own: the luma is a fixed sequence of fp32 roundings, the moments those of element-wise fp64 passes
// (window_f64.h, which says so per function; this covers the rest of the file)
#pragma clang fp contract(off)

// Bytes of fp64 planes the backward pass keeps at a time (at least one image's).  Not part of the ABI: a data symbol the tests shrink to
// drive the chunk loop with small images.
extern "C" {
size_t dcpt_ssim_loss_plane_cap = (size_t)64 << 20;
}

namespace {
constexpr int TH = METRIC_TH, TW = METRIC_TW, WIN = METRIC_WIN;
constexpr int SH = METRIC_SH, SW = METRIC_SW;   // staged rows / columns
constexpr int NT = METRIC_NT;

struct SsimGeom {
    int C, Cp;           // input channels, scored channels (1 for luma)
    int H, W, crop;
    int Hc, Wc;          // cropped size
    int Hm, Wm;          // SSIM-map size
    int nty, ntx;        // tiles of map positions
    int gty, gtx;        // tiles of input pixels (gather)
    int luma;
    double c1, c2;
};

constexpr float YR = 65.481f, YG = 128.553f, YB = 24.966f;

// the value SSIM is evaluated on: the fp32 input, or its luma Y = (((r 65.481f + g 128.553f) + b 24.966f) + 16.0f) / 255.0f, every product,
// sum and the division rounded to fp32 in this order (rgb2ycbcr_pt(y_only=True), basicsr/utils/color_util.py:222-254, is an fp32 matmul
// whose order of summation is not specified; this is the order torch's CPU matmul gives)
__device__ __forceinline__ float ssim_value(const float* __restrict__ img, int64_t plane, int64_t off, int luma) {
    if (!luma) return img[off];
    const float r = img[off], g = img[off + plane], b = img[off + 2 * plane];
    // plain operators under this file's contract(off): the __fmul_rn / __fadd_rn wrappers are header code compiled with contraction allowed,
    // and the products then fuse into the sums
    const float rg = r * YR + g * YG;
    const float rgb = rg + b * YB;
    return (rgb + 16.0f) / 255.0f;
}

// MAPS = false: part[blockIdx.y][tile] = sum of S over the tile.  MAPS = true: planes[blockIdx.y][3][Hm][Wm] = Pa, Pb, Pc.
// blockIdx.y = (image - b0) * Cp + channel.
template <bool MAPS>
__global__ __launch_bounds__(NT) void ssim_tile_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                       double* __restrict__ part, const double* __restrict__ gscale,
                                                       double* __restrict__ planes, SsimGeom m, Gauss gw, int b0) {
    __shared__ float sx[SH][SW], sy[SH][SW];
    __shared__ double hp[5][SH][TW];
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / m.ntx, tx = blockIdx.x - ty * m.ntx;
    const int bl = blockIdx.y / m.Cp, ch = blockIdx.y - bl * m.Cp, b = b0 + bl;
    const int64_t plane = (int64_t)m.H * m.W;
    const float* px = pred + ((int64_t)b * m.C + ch) * plane;
    const float* py = target + ((int64_t)b * m.C + ch) * plane;
    const int y0 = ty * TH, x0 = tx * TW;

    for (int i = tid; i < SH * SW; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 + r, gx = x0 + c;
        float vx = 0.f, vy = 0.f;
        if (gy < m.Hc && gx < m.Wc) {
            const int64_t off = (int64_t)(gy + m.crop) * m.W + (gx + m.crop);
            vx = ssim_value(px, plane, off, m.luma);
            vy = ssim_value(py, plane, off, m.luma);
        }
        sx[r][c] = vx;
        sy[r][c] = vy;
    }
    __syncthreads();
    const Gauss taps = gw;   // (a copy made here, where the passes start: window_f64.h)
    gauss_rows<float, SW>(sx, sy, hp, taps);
    __syncthreads();
    // ---- vertical pass, S and its partial derivatives ----
    const double w = MAPS ? gscale[(int64_t)b * m.Cp + ch] : 0.0;
    const int64_t msize = (int64_t)m.Hm * m.Wm;
    double* pa = MAPS ? planes + (int64_t)blockIdx.y * 3 * msize : nullptr;
    double acc = 0.0;
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        if (y0 + r >= m.Hm || x0 + c >= m.Wm) continue;
        const Moments o = gauss_col(hp, r, c, taps);
        const double mx = o.mu1, my = o.mu2;
        const double A1 = 2.0 * o.mu12 + m.c1, A2 = 2.0 * o.s12 + m.c2, B1 = o.mu1_sq + o.mu2_sq + m.c1, B2 = o.s1 + o.s2 + m.c2;
        const double S = (A1 / B1) * (A2 / B2);
        if (MAPS) {
            const double b12 = B1 * B2;
            const int64_t p = (int64_t)(y0 + r) * m.Wm + (x0 + c);
            pa[p] = w * (2.0 * my * (A2 - A1) / b12 - S * (2.0 * mx / B1 - 2.0 * mx / B2));
            pa[msize + p] = -(w * S / B2);
            pa[2 * msize + p] = 2.0 * w * A1 / b12;
        } else {
            acc += S;
        }
    }
    if (!MAPS) {
        acc = block_sum(acc, red);
        if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
    }
}

// one workgroup per TH x TW tile of input pixels of one (image, scored channel); blockIdx.y as in ssim_tile_kernel
__global__ __launch_bounds__(NT) void ssim_gather_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                         const double* __restrict__ planes, float* __restrict__ dpred, SsimGeom m, Gauss gw,
                                                         int b0) {
    __shared__ double sp[3][SH][SW];   // sp[.][r][c] = plane at map position (y0 - 10 + r, x0 - 10 + c)
    __shared__ double hq[3][SH][TW];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / m.gtx, tx = blockIdx.x - ty * m.gtx;
    const int bl = blockIdx.y / m.Cp, ch = blockIdx.y - bl * m.Cp, b = b0 + bl;
    const int64_t plane = (int64_t)m.H * m.W, msize = (int64_t)m.Hm * m.Wm;
    const int64_t img_off = ((int64_t)b * m.C + ch) * plane;
    const double* pl = planes + (int64_t)blockIdx.y * 3 * msize;
    const int y0 = ty * TH - m.crop, x0 = tx * TW - m.crop;   // the tile's origin in cropped coordinates (negative inside the border)

    for (int i = tid; i < SH * SW; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int my = y0 - (WIN - 1) + r, mx = x0 - (WIN - 1) + c;
        double va = 0.0, vb = 0.0, vc = 0.0;
        if (my >= 0 && my < m.Hm && mx >= 0 && mx < m.Wm) {
            const int64_t p = (int64_t)my * m.Wm + mx;
            va = pl[p];
            vb = pl[msize + p];
            vc = pl[2 * msize + p];
        }
        sp[0][r][c] = va;
        sp[1][r][c] = vb;
        sp[2][r][c] = vc;
    }
    __syncthreads();
    // ---- horizontal transposed pass: pixel column x0 + c gathers the map columns x0 + c - k ----
    for (int i = tid; i < SH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double g = gw.g[k];
            a0 += g * sp[0][r][c + (WIN - 1) - k];
            a1 += g * sp[1][r][c + (WIN - 1) - k];
            a2 += g * sp[2][r][c + (WIN - 1) - k];
        }
        hq[0][r][c] = a0;
        hq[1][r][c] = a1;
        hq[2][r][c] = a2;
    }
    __syncthreads();
    // ---- vertical transposed pass, combination with x and y, one rounding to fp32 ----
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        const int gy = ty * TH + r, gx = tx * TW + c;   // input coordinates
        if (gy >= m.H || gx >= m.W) continue;
        const int64_t off = (int64_t)gy * m.W + gx;
        const int qy = y0 + r, qx = x0 + c;
        double d = 0.0;
        const bool inside = qy >= 0 && qy < m.Hc && qx >= 0 && qx < m.Wc;
        if (inside) {
            double ga = 0.0, gb = 0.0, gc = 0.0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const double g = gw.g[k];
                ga += g * hq[0][r + (WIN - 1) - k][c];
                gb += g * hq[1][r + (WIN - 1) - k][c];
                gc += g * hq[2][r + (WIN - 1) - k][c];
            }
            const double x = (double)ssim_value(pred + img_off, plane, off, m.luma);
            const double y = (double)ssim_value(target + img_off, plane, off, m.luma);
            d = ga + 2.0 * x * gb + y * gc;
        }
        float* o = dpred + img_off + off;
        if (m.luma) {   // dY times (65.481f, 128.553f, 24.966f) / 255 in fp64, rounded once (0 stays exactly 0 in the border)
            o[0] = (float)(d * ((double)YR / 255.0));
            o[plane] = (float)(d * ((double)YG / 255.0));
            o[2 * plane] = (float)(d * ((double)YB / 255.0));
        } else {
            o[0] = (float)d;
        }
    }
}

SsimGeom ssim_geom(int C, int H, int W, int crop, int luma, double range) {
    SsimGeom m{};
    m.C = C;
    m.luma = luma && C == 3;
    m.Cp = m.luma ? 1 : C;
    m.H = H; m.W = W; m.crop = crop;
    m.Hc = H - 2 * crop; m.Wc = W - 2 * crop;
    m.Hm = m.Hc - (WIN - 1); m.Wm = m.Wc - (WIN - 1);
    m.nty = cdiv(m.Hm, TH); m.ntx = cdiv(m.Wm, TW);
    m.gty = cdiv(H, TH); m.gtx = cdiv(W, TW);
    m.c1 = (0.01 * range) * (0.01 * range);
    m.c2 = (0.03 * range) * (0.03 * range);
    return m;
}
}  // namespace

int ssim_loss_num_tiles(int Hc, int Wc) { return cdiv(Hc - (WIN - 1), TH) * cdiv(Wc - (WIN - 1), TW); }

size_t ssim_loss_plane_bytes(int Cp, int Hc, int Wc) { return (size_t)Cp * 3 * (size_t)(Hc - (WIN - 1)) * (size_t)(Wc - (WIN - 1)) * sizeof(double); }

int ssim_loss_chunk_images(int B, int Cp, int Hc, int Wc) {
    const size_t per = ssim_loss_plane_bytes(Cp, Hc, Wc);
    size_t n = dcpt_ssim_loss_plane_cap / per;
    if (n < 1) n = 1;
    return n > (size_t)B ? B : (int)n;
}

int launch_ssim_loss_fwd(const float* pred, const float* target, double* ssim_sum, double* part, int B, int C, int H, int W, int crop, int luma,
                         double range, hipStream_t s) {
    const SsimGeom m = ssim_geom(C, H, W, crop, luma, range);
    const Gauss gw = gauss_taps();
    const int ntiles = m.nty * m.ntx;
    trace_tag("ssim_loss.tile_fwd");
    ssim_tile_kernel<false><<<dim3((unsigned)ntiles, (unsigned)(B * m.Cp)), dim3(NT), 0, s>>>(pred, target, part, nullptr, nullptr, m, gw, 0);
    DCPT_CHECK_LAUNCH("ssim_loss_fwd tile");
    trace_tag("ssim_loss.reduce");
    sum_reduce_kernel<SUM_PLAIN><<<dim3((unsigned)(B * m.Cp)), dim3(NT), 0, s>>>(part, ssim_sum, ntiles, 1, 0);
    DCPT_CHECK_LAUNCH("ssim_loss_fwd reduce");
    return DCPT_OK;
}

int launch_ssim_loss_bwd(const float* pred, const float* target, const double* gscale, float* dpred, double* planes, int B, int C, int H, int W,
                         int crop, int luma, double range, hipStream_t s) {
    const SsimGeom m = ssim_geom(C, H, W, crop, luma, range);
    const Gauss gw = gauss_taps();
    const int chunk = ssim_loss_chunk_images(B, m.Cp, m.Hc, m.Wc);
    for (int b0 = 0; b0 < B; b0 += chunk) {   // (stream order: the gather of one chunk is done with the planes before the next map kernel)
        const int n = B - b0 < chunk ? B - b0 : chunk;
        trace_tag("ssim_loss.tile_bwd");
        ssim_tile_kernel<true><<<dim3((unsigned)(m.nty * m.ntx), (unsigned)(n * m.Cp)), dim3(NT), 0, s>>>(pred, target, nullptr, gscale, planes, m,
                                                                                                      gw, b0);
        DCPT_CHECK_LAUNCH("ssim_loss_bwd tile");
        trace_tag("ssim_loss.gather");
        ssim_gather_kernel<<<dim3((unsigned)(m.gty * m.gtx), (unsigned)(n * m.Cp)), dim3(NT), 0, s>>>(pred, target, planes, dpred, m, gw, b0);
        DCPT_CHECK_LAUNCH("ssim_loss_bwd gather");
    }
    return DCPT_OK;
}
