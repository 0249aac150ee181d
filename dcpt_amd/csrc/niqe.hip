// NIQE on the device (include/dcpt_hip.h dcpt_imresize_fwd, dcpt_niqe_mscn_fwd, dcpt_niqe_block_stats_fwd): the pixel work of
// basicsr/metrics/niqe.py and of basicsr/utils/matlab_functions.py::imresize in fp64; the 36 x 36 finish stays on the host.
//
//   resize       two element-wise passes, H then W as the reference: pass 1 writes the fp64 intermediate [P][Ho][W] into the workspace,
//                pass 2 the output.  A thread owns one output element and adds its K taps in table order.  The reference's symmetric
//                padded copy is addressing (index -1 -> 0, n -> n - 1); an index that would still leave the plane is clamped, so a
//                table the host layer would have refused cannot make the kernel read outside x.
//   MSCN         one workgroup per 16 x 32 output pixels of one plane: the (16 + 6) x (32 + 6) source values in LDS, the borders of
//                the cropped region replicated, then the 49 taps per pixel around the centre pixel p: s = sum w (x - p),
//                q = sum w (x - p)^2, var = q - s^2, n = -s / (sqrt|var| + 1).  A constant window gives n = 0 exactly.
//   block stats  one workgroup per (block, plane): a thread walks the block's elements tid, tid + 256, ... in row-major order, takes the
//                four rolled partners with wrapped indices from the plane (L2 hits: the block was just read) and keeps 5 x 6 sums; the
//                256 partials of each sum are added by a fixed tree.
// No atomics, every sum in a fixed order: two runs give the same bits, and a plane's result does not depend on its neighbours.
#include <math.h>

#include "kernels.h"
#include "prof.h"

namespace {
constexpr int NT = 256;
constexpr int TH = 16, TW = 32, R = 3, WIN = 7;
constexpr int SH = TH + 2 * R, SW = TW + 2 * R;

// the window is symmetric in |i|, |j| and their order: ten distinct weights (49 would not fit the scalar registers)
struct Window {
    double w[10];
};
constexpr int wslot(int a, int b) {
    const int i = a < R ? R - a : a - R, j = b < R ? R - b : b - R;
    const int u = i < j ? i : j, v = i < j ? j : i;
    return u * 4 - u * (u - 1) / 2 + (v - u);
}

// symmetric extension (index -1 -> 0, -2 -> 1, n -> n - 1, ...), then a clamp: never outside [0, n)
__device__ __forceinline__ int reflect(int i, int n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return min(max(i, 0), n - 1);
}

template <typename T>
__device__ __forceinline__ double tap(const T* __restrict__ p, int64_t off, int quant) {
    const T v = p[off];
    if (quant) return (double)rintf(__fmul_rn((float)v, 255.0f)) / 255.0;
    return (double)v;
}

// pass 1: t[p][i][x] = sum_k w_h[i][k] * X[p][reflect(first_h[i] + k)][x]
template <typename T>
__global__ __launch_bounds__(NT) void resize_h_kernel(const T* __restrict__ x, double* __restrict__ t, const int* __restrict__ first,
                                                      const double* __restrict__ wt, int64_t total, int H, int W, int Ho, int K,
                                                      int64_t plane_stride, int64_t row_stride, int quant) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const int col = (int)(e % W);
    const int64_t r = e / W;
    const int i = (int)(r % Ho);
    const int64_t p = r / Ho;
    const T* px = x + p * plane_stride + col;
    const double* wr = wt + (int64_t)i * K;
    const int f = first[i];
    double a = 0.0;
    for (int k = 0; k < K; ++k) a = fma(wr[k], tap(px, (int64_t)reflect(f + k, H) * row_stride, quant), a);
    t[e] = a;
}

// pass 2: y[p][i][j] = sum_k w_w[j][k] * t[p][i][reflect(first_w[j] + k)]; one rounding, at the store
template <typename T>
__global__ __launch_bounds__(NT) void resize_w_kernel(const double* __restrict__ t, T* __restrict__ y, const int* __restrict__ first,
                                                      const double* __restrict__ wt, int64_t total, int W, int Wo, int K) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e % Wo);
    const int64_t r = e / Wo;   // (plane, output row)
    const double* pt = t + r * W;
    const double* wr = wt + (int64_t)j * K;
    const int f = first[j];
    double a = 0.0;
    for (int k = 0; k < K; ++k) a = fma(wr[k], pt[reflect(f + k, W)], a);
    y[e] = (T)a;
}

// the cropped region of plane p starts at (crop, crop) of the [H][W] source and is Hc x Wc; n is [P][Hc][Wc]
template <typename T, bool Scale1>
__global__ __launch_bounds__(NT) void mscn_kernel(const T* __restrict__ x, double* __restrict__ n, int H, int W, int crop, int Hc, int Wc,
                                                  int ntx, Window g) {
    __shared__ double sx[SH][SW];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * TH, x0 = tx * TW;
    const T* px = x + (int64_t)blockIdx.y * H * W;
    for (int i = tid; i < SH * SW; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int gy = min(max(y0 + r - R, 0), Hc - 1), gx = min(max(x0 + c - R, 0), Wc - 1);   // scipy's mode="nearest"
        const T v = px[(int64_t)(gy + crop) * W + (gx + crop)];
        if (Scale1) {
            sx[r][c] = (double)rintf(__fmul_rn((float)v, 255.0f));   // (img * 255.0).round() of the float32 image, half to even
        } else {
            sx[r][c] = (double)v * 255.0;
        }
    }
    __syncthreads();
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        if (y0 + r >= Hc || x0 + c >= Wc) continue;
        const double p = sx[r + R][c + R];
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int a = 0; a < WIN; ++a) {
#pragma unroll
            for (int b = 0; b < WIN; ++b) {
                const double d = sx[r + a][c + b] - p, wd = g.w[wslot(a, b)] * d;
                s += wd;
                q = fma(wd, d, q);
            }
        }
        const double var = q - s * s;
        n[((int64_t)blockIdx.y * Hc + (y0 + r)) * Wc + (x0 + c)] = -s / (sqrt(fabs(var)) + 1.0);
    }
}

// six sums of one map: count and sum of squares of the negative elements, of the positive elements, sum |x| and sum x^2 over all
struct Six {
    double v[6];
};
__device__ __forceinline__ void add6(Six& a, double x) {
    const double x2 = x * x;
    if (x < 0.0) {
        a.v[0] += 1.0;
        a.v[1] += x2;
    }
    if (x > 0.0) {
        a.v[2] += 1.0;
        a.v[3] += x2;
    }
    a.v[4] += fabs(x);
    a.v[5] += x2;
}

__global__ __launch_bounds__(NT) void block_stats_kernel(const double* __restrict__ n, double* __restrict__ out, int H, int W, int bs,
                                                         int nbh) {
    __shared__ double red[6][NT];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;                     // the reference's order: idx_w outer, idx_h inner
    const int bw = blk / nbh, bh = blk - bw * nbh;
    const double* pn = n + (int64_t)blockIdx.y * H * W + (int64_t)bh * bs * W + (int64_t)bw * bs;
    Six acc[5];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[m].v[k] = 0.0;
    for (int e = tid; e < bs * bs; e += NT) {
        const int i = e / bs, j = e - i * bs;
        const int iu = i == 0 ? bs - 1 : i - 1, jl = j == 0 ? bs - 1 : j - 1, jr = j == bs - 1 ? 0 : j + 1;
        const double x = pn[(int64_t)i * W + j];
        add6(acc[0], x);
        add6(acc[1], x * pn[(int64_t)i * W + jl]);    // np.roll(block, [0, 1]):  (i, j) meets (i, j - 1)
        add6(acc[2], x * pn[(int64_t)iu * W + j]);    // [1, 0]:  (i - 1, j)
        add6(acc[3], x * pn[(int64_t)iu * W + jl]);   // [1, 1]:  (i - 1, j - 1)
        add6(acc[4], x * pn[(int64_t)iu * W + jr]);   // [1, -1]: (i - 1, j + 1)
    }
    double* po = out + ((int64_t)blockIdx.y * gridDim.x + blk) * 30;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[k][tid] = acc[m].v[k];
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {   // fixed tree over the 256 partials
            if (tid < s) {
#pragma unroll
                for (int k = 0; k < 6; ++k) red[k][tid] += red[k][tid + s];
            }
            __syncthreads();
        }
        if (tid < 6) po[m * 6 + tid] = red[tid][0];
        __syncthreads();
    }
}

unsigned blocks_for(int64_t total) { return (unsigned)cdiv64(total, NT); }
}  // namespace

int launch_imresize_fwd(const void* x, void* y, const int* first_h, const double* w_h, const int* first_w, const double* w_w, double* t, int P,
                        int H, int W, int Ho, int Wo, int Kh, int Kw, int64_t plane_stride, int64_t row_stride, int x_f64, int y_f64,
                        int quant, hipStream_t s) {
    const int64_t n1 = (int64_t)P * Ho * W, n2 = (int64_t)P * Ho * Wo;
    trace_tag("imresize.h");
    if (x_f64) {
        resize_h_kernel<double><<<dim3(blocks_for(n1)), dim3(NT), 0, s>>>((const double*)x, t, first_h, w_h, n1, H, W, Ho, Kh, plane_stride,
                                                                         row_stride, 0);
    } else {
        resize_h_kernel<float><<<dim3(blocks_for(n1)), dim3(NT), 0, s>>>((const float*)x, t, first_h, w_h, n1, H, W, Ho, Kh, plane_stride,
                                                                        row_stride, quant);
    }
    DCPT_CHECK_LAUNCH("imresize h pass");
    trace_tag("imresize.w");
    if (y_f64) {
        resize_w_kernel<double><<<dim3(blocks_for(n2)), dim3(NT), 0, s>>>(t, (double*)y, first_w, w_w, n2, W, Wo, Kw);
    } else {
        resize_w_kernel<float><<<dim3(blocks_for(n2)), dim3(NT), 0, s>>>(t, (float*)y, first_w, w_w, n2, W, Wo, Kw);
    }
    DCPT_CHECK_LAUNCH("imresize w pass");
    return DCPT_OK;
}

int launch_niqe_mscn_fwd(const void* x, double* n, int P, int H, int W, int crop, int Hc, int Wc, int scale, hipStream_t s) {
    Window g;   // exp(-(i^2 + j^2) / (2 (7/6)^2)), normalised: the reference's stored gaussian_window to 1.4e-17
    const double sigma = 7.0 / 6.0;
    double full[WIN * WIN], sum = 0.0;
    for (int a = 0; a < WIN; ++a)
        for (int b = 0; b < WIN; ++b) {
            const double i = a - R, j = b - R;
            full[a * WIN + b] = exp(-(i * i + j * j) / (2.0 * sigma * sigma));
            sum += full[a * WIN + b];
        }
    for (int a = 0; a < WIN; ++a)
        for (int b = 0; b < WIN; ++b) g.w[wslot(a, b)] = full[a * WIN + b] / sum;
    const int nty = cdiv(Hc, TH), ntx = cdiv(Wc, TW);
    const dim3 grid((unsigned)(nty * ntx), (unsigned)P);
    trace_tag(scale == 1 ? "niqe.mscn1" : "niqe.mscn2");
    if (scale == 1) {
        mscn_kernel<float, true><<<grid, dim3(NT), 0, s>>>((const float*)x, n, H, W, crop, Hc, Wc, ntx, g);
    } else {
        mscn_kernel<double, false><<<grid, dim3(NT), 0, s>>>((const double*)x, n, H, W, crop, Hc, Wc, ntx, g);
    }
    DCPT_CHECK_LAUNCH("niqe mscn");
    return DCPT_OK;
}

int launch_niqe_block_stats_fwd(const double* n, double* stats, int P, int H, int W, int block, hipStream_t s) {
    const int nbh = H / block, nbw = W / block;
    trace_tag(block == 96 ? "niqe.stats96" : "niqe.stats48");
    block_stats_kernel<<<dim3((unsigned)(nbh * nbw), (unsigned)P), dim3(NT), 0, s>>>(n, stats, H, W, block, nbh);
    DCPT_CHECK_LAUNCH("niqe block stats");
    return DCPT_OK;
}
