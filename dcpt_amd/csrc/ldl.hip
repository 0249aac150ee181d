// The LDL artifact-weight map on the device (include/dcpt_hip.h dcpt_ldl_weight_fwd / dcpt_ldl_weight_bwd): the only path of the reference's
// get_refined_artifact_map (basicsr/losses/loss_util.py:100-165) that SRModel.optimize_parameters (basicsr/models/sr_model.py:145-153)
// reaches -- std=True, ksize 7, no img_ema -- and its gradient with respect to the output image, without the reference's 49-fold unfold
// of the residual.  gt, out: fp32 NCHW [B][C][H][W]; N = B C H W.
//     r = |gt - out|
//     u = unbiased std of r over the 7 x 7 window around each pixel, r reflect-padded by 3 (divide by 48)
//     m = mean(u), s = unbiased std(u) over all N elements
//     w = (tanh((u - m) / s) + 1) / 2
// and, given Gw = dL/dw, with t = tanh z, z = (u - m) / s:
//     Gz = Gw (1 - t^2) / 2
//     Gu = (Gz - sum(Gz) / N - z sum(Gz z) / (N - 1)) / s
//     Gv = Gu / (2 u), 0 where u == 0 (as torch's std backward masks it)
//     Gr = (2 / 48) (r T(Gv) - T(Gv mu)),  mu the window mean of r
//     Gout = Gr sign(out - gt)
// T is the transpose of "reflect-pad by 3, then 7 x 7 box": per axis, the 7-tap box sum over the padded domain [-3, W + 2] of a plane that
// is zero outside [0, W), folded back by q < 0 -> -q and q >= W -> 2 (W - 1) - q.  A pixel j receives the padded positions j, -j
// (1 <= j <= 3) and 2 (W - 1) - j (W - 4 <= j <= W - 2): a gather over at most three positions per axis; for W in 4..6 both folds land on
// the same pixels.
//
// Everything is fp64.  The one departure from the reference: r is |double(gt) - double(out)|, the exact difference of the two fp32 values,
// where the reference rounds the difference to fp32 first.  w and the gradient are rounded once to fp32.
//
// Forward, five launches: (1) one workgroup per TH x TW tile of one (image, channel) plane stages r with its 3-wide halo in LDS (the halo
// by reflect addressing: no padded copy exists), runs the separable box pass of r - pivot and (r - pivot)^2, writes u and mu as fp64
// planes and one partial of sum(u); the pivot is the smallest r of the staged tile: sums of shifted values do not cancel the way raw
// sum(r^2) - sum(r)^2 / 49 does on a smooth residual, and, r being non-negative, a tile that holds an all-zero window has pivot 0, so that
// window's u is exactly 0; (2) one workgroup adds the partials in a fixed order (sum_reduce_kernel of block_sum.h, whose tree every block
// sum and the pivot's minimum here go through as well): m; (3) sum((u - m)^2) per chunk of CHUNK elements;
// (4) the same reduce kernel: s; (5) w.  Backward, four launches: (1) Gz per element and the partials of sum(Gz), sum(Gz z) per chunk;
// (2) the reduce kernel; (3) the planes Gv and Gv mu; (4) one workgroup per TH x TW tile of input pixels stages both planes with a 3-wide
// zero halo, runs T as two separable gather passes, combines with r and the sign and writes Gout.  m, s and the two sums stay in the
// workspace: nothing is read back.  No atomics, every sum in a fixed order: the same input gives the same bits.
//
// out == gt everywhere gives u = 0, m = 0, s = 0, z = 0 / 0: w is NaN everywhere, which is what the reference's expression gives.
#include <math.h>

#include "block_sum.h"
#include "kernels.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {
constexpr int TH = METRIC_TH, TW = METRIC_TW, WIN = 7, PAD = 3;
constexpr int SH = TH + WIN - 1, SW = TW + WIN - 1;   // staged rows / columns
constexpr int NT = BLOCK_NT;
constexpr int CHUNK = LDL_CHUNK;                      // elements per workgroup of the element-wise kernels that leave a partial

struct LdlGeom {
    int H, W;
    int nty, ntx;
    int64_t N;
};

__device__ __forceinline__ int reflect(int q, int n) { return q < 0 ? -q : (q >= n ? 2 * (n - 1) - q : q); }

// one workgroup per TH x TW tile of the plane blockIdx.y = image * C + channel
__global__ __launch_bounds__(NT) void ldl_tile_kernel(const float* __restrict__ gt, const float* __restrict__ out, double* __restrict__ u,
                                                      double* __restrict__ mu, double* __restrict__ part, LdlGeom m) {
    __shared__ double sr[SH][SW];      // sr[r][c] = r at padded position (y0 - 3 + r, x0 - 3 + c), reflected into the plane
    __shared__ double hp[2][SH][TW];
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / m.ntx, tx = blockIdx.x - ty * m.ntx;
    const int64_t base = (int64_t)blockIdx.y * m.H * m.W;
    const int y0 = ty * TH, x0 = tx * TW;

    double lo = INFINITY;
    for (int i = tid; i < SH * SW; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int qy = y0 - PAD + r, qx = x0 - PAD + c;
        double v = 0.0;
        if (qy < m.H + PAD && qx < m.W + PAD) {   // (past the padded plane in a ragged tile: nothing reads it)
            const int64_t off = base + (int64_t)reflect(qy, m.H) * m.W + reflect(qx, m.W);
            v = fabs((double)gt[off] - (double)out[off]);
            lo = fmin(lo, v);
        }
        sr[r][c] = v;
    }
    const double pivot = block_tree(lo, red, [](double a, double b) { return fmin(a, b); });   // (finite: the tile's first pixel is in the plane)
    // ---- horizontal pass of r - pivot and its square ----
    for (int i = tid; i < SH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double d = sr[r][c + k] - pivot;
            a1 += d;
            a2 += d * d;
        }
        hp[0][r][c] = a1;
        hp[1][r][c] = a2;
    }
    __syncthreads();
    // ---- vertical pass, u and mu ----
    double acc = 0.0;
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        if (y0 + r >= m.H || x0 + c >= m.W) continue;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            s1 += hp[0][r + k][c];
            s2 += hp[1][r + k][c];
        }
        const double var = (s2 - s1 * s1 / 49.0) / 48.0;
        const double sd = var > 0.0 ? sqrt(var) : 0.0;
        const int64_t p = base + (int64_t)(y0 + r) * m.W + (x0 + c);
        u[p] = sd;
        mu[p] = pivot + s1 / 49.0;
        acc += sd;
    }
    acc = block_sum(acc, red);
    if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// part[blockIdx.x] = sum over the workgroup's CHUNK elements of (u - m)^2
__global__ __launch_bounds__(NT) void ldl_dev_kernel(const double* __restrict__ u, const double* __restrict__ scal, double* __restrict__ part,
                                                     int64_t N) {
    __shared__ double red[NT];
    const double mean = scal[0];
    const int64_t i0 = (int64_t)blockIdx.x * CHUNK;
    double a = 0.0;
    for (int k = threadIdx.x; k < CHUNK; k += NT) {
        const int64_t i = i0 + k;
        if (i < N) {
            const double d = u[i] - mean;
            a += d * d;
        }
    }
    a = block_sum(a, red);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

__global__ __launch_bounds__(NT) void ldl_w_kernel(const double* __restrict__ u, const double* __restrict__ scal, float* __restrict__ w,
                                                   int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    w[i] = (float)((tanh((u[i] - scal[0]) / scal[1]) + 1.0) / 2.0);
}

// Gz of element i and its z
__device__ __forceinline__ double ldl_gz(double u, double gw, double mean, double sd, double* z) {
    *z = (u - mean) / sd;
    const double t = tanh(*z);
    return gw * (1.0 - t * t) / 2.0;
}

// part[blockIdx.x] = sum of Gz, part[np + blockIdx.x] = sum of Gz z over the workgroup's CHUNK elements
__global__ __launch_bounds__(NT) void ldl_gz_kernel(const double* __restrict__ u, const float* __restrict__ gw, const double* __restrict__ scal,
                                                    double* __restrict__ part, int64_t np, int64_t N) {
    __shared__ double red[NT];
    const double mean = scal[0], sd = scal[1];
    const int64_t i0 = (int64_t)blockIdx.x * CHUNK;
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < CHUNK; k += NT) {
        const int64_t i = i0 + k;
        if (i < N) {
            double z;
            const double g = ldl_gz(u[i], (double)gw[i], mean, sd, &z);
            a += g;
            b += g * z;
        }
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a;
        part[np + blockIdx.x] = b;
    }
}

// gv = Gv, gvmu = Gv mu
__global__ __launch_bounds__(NT) void ldl_gv_kernel(const double* __restrict__ u, const double* __restrict__ mu, const float* __restrict__ gw,
                                                    const double* __restrict__ scal, double* __restrict__ gv, double* __restrict__ gvmu,
                                                    int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const double sd = scal[1], ui = u[i];
    double z;
    const double g = ldl_gz(ui, (double)gw[i], scal[0], sd, &z);
    const double gu = (g - scal[2] / (double)N - z * scal[3] / (double)(N - 1)) / sd;
    const double v = ui == 0.0 ? 0.0 : gu / (2.0 * ui);
    gv[i] = v;
    gvmu[i] = v * mu[i];
}

// The positions lo .. hi (clipped to the plane [0, n)) of the 7-tap box around the padded position q, as a half-open range of staged
// indices: staged index = position - origin + PAD.
struct Taps {
    int lo, hi;
};
__device__ __forceinline__ Taps box_taps(int q, int n, int origin) {
    const int lo = q - PAD < 0 ? 0 : q - PAD, hi = q + PAD > n - 1 ? n - 1 : q + PAD;
    return {lo - origin + PAD, hi - origin + PAD + 1};
}

// one workgroup per TH x TW tile of input pixels of the plane blockIdx.y
__global__ __launch_bounds__(NT) void ldl_gather_kernel(const float* __restrict__ gt, const float* __restrict__ out,
                                                        const double* __restrict__ gv, const double* __restrict__ gvmu,
                                                        float* __restrict__ dout, LdlGeom m) {
    __shared__ double sp[2][SH][SW];   // sp[.][r][c] = plane at (y0 - 3 + r, x0 - 3 + c), zero outside the plane
    __shared__ double hq[2][SH][TW];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / m.ntx, tx = blockIdx.x - ty * m.ntx;
    const int64_t base = (int64_t)blockIdx.y * m.H * m.W;
    const int y0 = ty * TH, x0 = tx * TW;

    for (int i = tid; i < SH * SW; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int py = y0 - PAD + r, px = x0 - PAD + c;
        double a = 0.0, b = 0.0;
        if (py >= 0 && py < m.H && px >= 0 && px < m.W) {
            const int64_t p = base + (int64_t)py * m.W + px;
            a = gv[p];
            b = gvmu[p];
        }
        sp[0][r][c] = a;
        sp[1][r][c] = b;
    }
    __syncthreads();
    // ---- horizontal transposed pass: pixel column j gathers the boxes around the padded columns j, -j and 2 (W - 1) - j ----
    for (int i = tid; i < SH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        const int j = x0 + c;
        double a = 0.0, b = 0.0;
        if (j < m.W) {
            const int q[3] = {j, -j, 2 * (m.W - 1) - j};
            const bool use[3] = {true, j >= 1 && j <= PAD, j >= m.W - 1 - PAD && j <= m.W - 2};
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                if (!use[f]) continue;
                const Taps t = box_taps(q[f], m.W, x0);   // (staged columns 0 .. SW - 1: the taps lie within 3 of j)
                for (int k = t.lo; k < t.hi; ++k) {
                    a += sp[0][r][k];
                    b += sp[1][r][k];
                }
            }
        }
        hq[0][r][c] = a;
        hq[1][r][c] = b;
    }
    __syncthreads();
    // ---- vertical transposed pass, combination with r and the sign, one rounding to fp32 ----
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= m.H || gx >= m.W) continue;
        const int q[3] = {gy, -gy, 2 * (m.H - 1) - gy};
        const bool use[3] = {true, gy >= 1 && gy <= PAD, gy >= m.H - 1 - PAD && gy <= m.H - 2};
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            if (!use[f]) continue;
            const Taps t = box_taps(q[f], m.H, y0);
            for (int k = t.lo; k < t.hi; ++k) {
                a += hq[0][k][c];
                b += hq[1][k][c];
            }
        }
        const int64_t p = base + (int64_t)gy * m.W + gx;
        const double d = (double)out[p] - (double)gt[p];
        const double gr = (2.0 / 48.0) * (fabs(d) * a - b);
        dout[p] = (float)(d > 0.0 ? gr : (d < 0.0 ? -gr : 0.0));
    }
}

LdlGeom ldl_geom(int B, int C, int H, int W) {
    LdlGeom m{};
    m.H = H; m.W = W;
    m.nty = cdiv(H, TH); m.ntx = cdiv(W, TW);
    m.N = (int64_t)B * C * H * W;
    return m;
}
}  // namespace

int64_t ldl_num_partials(int B, int C, int H, int W) {
    const int64_t tiles = (int64_t)B * C * cdiv(H, TH) * cdiv(W, TW), chunks = cdiv64((int64_t)B * C * H * W, CHUNK);
    return tiles > chunks ? tiles : chunks;
}

int launch_ldl_weight_fwd(const float* gt, const float* out, float* w, const LdlWs& ws, int B, int C, int H, int W, hipStream_t s) {
    const LdlGeom m = ldl_geom(B, C, H, W);
    const int ntiles = m.nty * m.ntx;
    const unsigned chunks = (unsigned)cdiv64(m.N, CHUNK), ew = (unsigned)cdiv64(m.N, NT);
    trace_tag("ldl.tile");
    ldl_tile_kernel<<<dim3((unsigned)ntiles, (unsigned)(B * C)), dim3(NT), 0, s>>>(gt, out, ws.u, ws.mu, ws.part, m);
    DCPT_CHECK_LAUNCH("ldl_weight_fwd tile");
    trace_tag("ldl.reduce");
    sum_reduce_kernel<SUM_MEAN><<<dim3(1), dim3(NT), 0, s>>>(ws.part, ws.scal, (int64_t)B * C * ntiles, 1, m.N);
    DCPT_CHECK_LAUNCH("ldl_weight_fwd mean");
    trace_tag("ldl.dev");
    ldl_dev_kernel<<<dim3(chunks), dim3(NT), 0, s>>>(ws.u, ws.scal, ws.part, m.N);
    DCPT_CHECK_LAUNCH("ldl_weight_fwd dev");
    trace_tag("ldl.reduce");
    sum_reduce_kernel<SUM_STD><<<dim3(1), dim3(NT), 0, s>>>(ws.part, ws.scal + 1, (int64_t)chunks, 1, m.N);
    DCPT_CHECK_LAUNCH("ldl_weight_fwd std");
    trace_tag("ldl.w");
    ldl_w_kernel<<<dim3(ew), dim3(NT), 0, s>>>(ws.u, ws.scal, w, m.N);
    DCPT_CHECK_LAUNCH("ldl_weight_fwd w");
    return DCPT_OK;
}

int launch_ldl_weight_bwd(const float* gt, const float* out, const float* gw, float* dout, const LdlWs& ws, int B, int C, int H, int W,
                          hipStream_t s) {
    const LdlGeom m = ldl_geom(B, C, H, W);
    const unsigned chunks = (unsigned)cdiv64(m.N, CHUNK), ew = (unsigned)cdiv64(m.N, NT);
    trace_tag("ldl.gz");
    ldl_gz_kernel<<<dim3(chunks), dim3(NT), 0, s>>>(ws.u, gw, ws.scal, ws.part, (int64_t)chunks, m.N);
    DCPT_CHECK_LAUNCH("ldl_weight_bwd gz");
    trace_tag("ldl.reduce");
    sum_reduce_kernel<SUM_PLAIN><<<dim3(2), dim3(NT), 0, s>>>(ws.part, ws.scal + 2, (int64_t)chunks, 1, m.N);   // (the two rows of part)
    DCPT_CHECK_LAUNCH("ldl_weight_bwd sums");
    trace_tag("ldl.gv");
    ldl_gv_kernel<<<dim3(ew), dim3(NT), 0, s>>>(ws.u, ws.mu, gw, ws.scal, ws.gv, ws.gvmu, m.N);
    DCPT_CHECK_LAUNCH("ldl_weight_bwd gv");
    trace_tag("ldl.gather");
    ldl_gather_kernel<<<dim3((unsigned)(m.nty * m.ntx), (unsigned)(B * C)), dim3(NT), 0, s>>>(gt, out, ws.gv, ws.gvmu, dout, m);
    DCPT_CHECK_LAUNCH("ldl_weight_bwd gather");
    return DCPT_OK;
}
