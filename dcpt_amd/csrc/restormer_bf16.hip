// Restormer blocks with bf16 activation storage (reference basicsr/archs/restormer_arch.py), the decomposition of restormer.hip:
//   MDTA  x + project_out(attn(LN(x)))  (:103-145, :148-159)   dcpt_mdta_bf16_fwd/bwd
//   GDFN  x + project_out(gelu(x1)*x2)  (:75-100)              dcpt_gdfn_bf16_fwd/bwd
// plus the NHWC glue between blocks in bf16: PixelShuffle/PixelUnshuffle(2) (:175-202) and channel concat / split (:390-400).
//
// Every feature map between the blocks and every tensor a block keeps for backward is bf16 (rounded once, on store, RNE); the
// LayerNorm statistics, the L2 norms, the Gram / attention matrices and their gradients, the parameters and all parameter
// gradients stay fp32, and every sum is accumulated in fp32.  The 1 x 1 convs run on the bf16 NT / TN GEMMs (gemm_bf16.hip), the
// GDFN depthwise + gate and its backward on the bf16 row ring (dwring.hip); the MDTA depthwise (forward with the sums of squares of
// q / k, and backward) has a register kernel of its own here.  The per-(image, head) products are ch x ch
// with ch = C / heads (48 in the default net) -- too narrow for the GEMM tiles -- and have two kernels of their own here:
//   gram   G[i][j]  = sum_p X[p][i] Y[p][j]             over fixed 256-pixel splits (fp32 slabs, reduced in order by the finalize)
//   apply  O[p][i]  = sum_j A[i][j] V[p][j] (+ cs_i R[p][i])   A in LDS (fp32), a 32-pixel tile of V next to it
// for heads of up to 96 channels; wider heads (up to 256: PromptIR's noise_level3 has 176) run tiled forms of the two (*_wide_bf16_kernel).
// The attention finalize / backward (ReLU or softmax, temperature, norms) are the fp32 kernels of restormer.hip.  Nothing is
// accumulated with atomics, and no split depends on the batch size: a sample's output does not depend on its batch.
#include "bf16.h"
#include "bf16_ops.h"
#include "kernels.h"
#include "prof.h"
#include "../../include/dcpt_hip.h"

namespace {

__device__ __forceinline__ float bf2f(bf16_t v) { return bf_lo((uint32_t)v); }
__device__ __forceinline__ bf16_t f2bf(float v) { return (bf16_t)(bf_pack(v, 0.f) & 0xffffu); }

// ---- LayerNorm over bf16 rows (one wave per row, fp32 statistics two-pass) -----------------------------------------------
// WithBias (:43-59):  y = (x - mu) * rstd * w + b;   BiasFree (:26-40):  y = x * rstd * w  (variance about the mean, mean kept)
constexpr int LN_MAXJ = 16;   // C <= 1024
template <bool BF>
__global__ __launch_bounds__(256) void ln_fwd_rows_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                          bf16_t* __restrict__ y, float* __restrict__ mu, float* __restrict__ rstd, int64_t M,
                                                          int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const bf16_t* xr = x + m * C;
    float v[LN_MAXJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < C ? bf2f(xr[c]) : 0.f;
        s += v[j];
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int c = lane + 64 * j;
        const float d = c < C ? v[j] - mean : 0.f;
        q = fmaf(d, d, q);
    }
    const float r = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
    bf16_t* yr = y + m * C;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int c = lane + 64 * j;
        if (c < C) yr[c] = f2bf(BF ? v[j] * r * w[c] : fmaf((v[j] - mean) * r, w[c], b[c]));
    }
    if (lane == 0) {
        mu[m] = mean;
        rstd[m] = r;
    }
}

// backward: g = the gradient of the LayerNorm output (bf16), dres = the residual's gradient; dx = LN'(g) + dres.  A wave owns a contiguous
// row range and writes its parameter partials part[wave][0][c] = sum g * xhat (xhat = (x - mu) rstd, BiasFree: x rstd), part[wave][1][c] = sum g.
//   WithBias:  dx = rstd (g w - mean(g w) - xhat mean(g w xhat));   BiasFree:  dx = rstd g w - rstd^3 (x - mu) mean(g w x)
template <bool BF>
__global__ __launch_bounds__(256) void ln_bwd_rows_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ x, const float* __restrict__ mu,
                                                          const float* __restrict__ rstd, const float* __restrict__ w, const bf16_t* __restrict__ dres,
                                                          bf16_t* __restrict__ dx, float* __restrict__ part, int64_t M, int C, int64_t rpw) {
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    float pw[LN_MAXJ], pb[LN_MAXJ];
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) pw[j] = pb[j] = 0.f;
    const int64_t m0 = wv * rpw, m1 = m0 + rpw < M ? m0 + rpw : M;
    for (int64_t m = m0; m < m1; ++m) {
        const float mean = mu[m], r = rstd[m];
        float gv[LN_MAXJ], xv[LN_MAXJ];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < LN_MAXJ; ++j) {
            const int c = lane + 64 * j;
            gv[j] = c < C ? bf2f(g[m * C + c]) : 0.f;
            xv[j] = c < C ? bf2f(x[m * C + c]) : 0.f;
            const float gw = c < C ? gv[j] * w[c] : 0.f;
            const float xh = BF ? xv[j] * r : (xv[j] - mean) * r;
            s1 += gw;
            s2 = fmaf(gw, BF ? xv[j] : xh, s2);
            pw[j] = fmaf(gv[j], xh, pw[j]);
            pb[j] += gv[j];
        }
        s1 = wave_sum(s1) / (float)C;
        s2 = wave_sum(s2) / (float)C;
#pragma unroll
        for (int j = 0; j < LN_MAXJ; ++j) {
            const int c = lane + 64 * j;
            if (c < C) {
                const float gw = gv[j] * w[c];
                const float d = BF ? r * gw - r * r * r * (xv[j] - mean) * s2 : r * (gw - s1 - (xv[j] - mean) * r * s2);
                dx[m * C + c] = f2bf(d + (dres ? bf2f(dres[m * C + c]) : 0.f));
            }
        }
    }
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int c = lane + 64 * j;
        if (c < C) {
            part[(wv * 2 + 0) * C + c] = pw[j];
            part[(wv * 2 + 1) * C + c] = pb[j];
        }
    }
}

constexpr int LN_BWD_WAVES = 2048;
int ln_bwd_waves(int64_t M) { return (int)(M < LN_BWD_WAVES ? (M + 3) / 4 * 4 : LN_BWD_WAVES); }

int launch_ln_fwd_rows(const bf16_t* x, const float* w, const float* b, bf16_t* y, float* mu, float* rstd, int64_t M, int C, float eps,
                       bool biasfree, hipStream_t s) {
    trace_tag("rst_bf16.ln_fwd");
    const dim3 grid((unsigned)cdiv64(M, 4)), blk(256);
    if (biasfree) ln_fwd_rows_kernel<true><<<grid, blk, 0, s>>>(x, w, b, y, mu, rstd, M, C, eps);
    else ln_fwd_rows_kernel<false><<<grid, blk, 0, s>>>(x, w, b, y, mu, rstd, M, C, eps);
    DCPT_CHECK_LAUNCH("rst_bf16_ln_fwd");
    return DCPT_OK;
}

// part: [ln_bwd_waves(M)][2][C]
int launch_ln_bwd_rows(const bf16_t* g, const bf16_t* x, const float* mu, const float* rstd, const float* w, const bf16_t* dres, bf16_t* dx,
                       float* part, int64_t M, int C, bool biasfree, hipStream_t s) {
    trace_tag("rst_bf16.ln_bwd");
    const int nw = ln_bwd_waves(M);
    const int64_t rpw = cdiv64(M, nw);
    const dim3 grid((unsigned)(nw / 4)), blk(256);
    if (biasfree) ln_bwd_rows_kernel<true><<<grid, blk, 0, s>>>(g, x, mu, rstd, w, dres, dx, part, M, C, rpw);
    else ln_bwd_rows_kernel<false><<<grid, blk, 0, s>>>(g, x, mu, rstd, w, dres, dx, part, M, C, rpw);
    DCPT_CHECK_LAUNCH("rst_bf16_ln_bwd");
    return DCPT_OK;
}

// ---- MDTA depthwise 3x3 over the 3C qkv channels (no bias) + per-(image, row) sums of squares of the rounded q / k outputs -----
// A thread owns 8 channels of one image row and slides along it (three input rows x three columns in registers).
// sqpart[b][h][2C] (channels < 2C: q and k).
__global__ __launch_bounds__(256) void dw_sq_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w2p, bf16_t* __restrict__ y,
                                                        float* __restrict__ sqpart, int B, int H, int W, int C3, int C2) {
    const int G = C3 / 8;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)B * H * G) return;
    const int gq = (int)(t % G);
    const int64_t bh = t / G;
    const int h = (int)(bh % H), b = (int)(bh / H);
    const int c0 = gq * 8;
    float wt[9][8];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) wt[k][e] = w2p[k * C3 + c0 + e];
    auto load = [&](int yy, int xx, float* o) {
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.f;
            return;
        }
        const u32x4 v = *reinterpret_cast<const u32x4*>(x + (((int64_t)b * H + yy) * W + xx) * C3 + c0);
        o[0] = bf_lo(v.x); o[1] = bf_hi(v.x); o[2] = bf_lo(v.y); o[3] = bf_hi(v.y);
        o[4] = bf_lo(v.z); o[5] = bf_hi(v.z); o[6] = bf_lo(v.w); o[7] = bf_hi(v.w);
    };
    float win[3][3][8];   // [ky][column x-1, x, x+1][e]
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        load(h + ky - 1, -1, win[ky][0]);
        load(h + ky - 1, 0, win[ky][1]);
    }
    float sq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sq[e] = 0.f;
    for (int xx = 0; xx < W; ++xx) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) load(h + ky - 1, xx + 1, win[ky][2]);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) a = fmaf(wt[ky * 3 + kx][e], win[ky][kx][e], a);
            o[e] = bf_round(a);
            sq[e] = fmaf(o[e], o[e], sq[e]);
        }
        u32x4 wv;
        wv.x = bf_pack(o[0], o[1]); wv.y = bf_pack(o[2], o[3]); wv.z = bf_pack(o[4], o[5]); wv.w = bf_pack(o[6], o[7]);
        *reinterpret_cast<u32x4*>(y + (((int64_t)b * H + h) * W + xx) * C3 + c0) = wv;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                win[ky][0][e] = win[ky][1][e];
                win[ky][1][e] = win[ky][2][e];
            }
    }
    if (c0 < C2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sqpart[((int64_t)b * H + h) * C2 + c0 + e] = sq[e];
    }
}

// ---- MDTA depthwise backward (plain, no bias), the same thread map: dx = the transposed conv of dy; tap gradients per (image, row):
// wpart[b H + h][t][c] = sum_x dy[h][x][c] in[h + ky - 1][x + kx - 1][c] (t = 3 ky + kx; row 9 = sum dy), reduced by launch_dw_wgrad_reduce
__global__ __launch_bounds__(256) void dw_plain_bwd_dx_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ w2p, bf16_t* __restrict__ dx,
                                                              int B, int H, int W, int C3) {
    const int G = C3 / 8;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)B * H * G) return;
    const int gq = (int)(t % G);
    const int64_t bh = t / G;
    const int h = (int)(bh % H), b = (int)(bh / H);
    const int c0 = gq * 8;
    auto load = [&](int yy, int xx, float* o) {
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.f;
            return;
        }
        const u32x4 v = *reinterpret_cast<const u32x4*>(dy + (((int64_t)b * H + yy) * W + xx) * C3 + c0);
        o[0] = bf_lo(v.x); o[1] = bf_hi(v.x); o[2] = bf_lo(v.y); o[3] = bf_hi(v.y);
        o[4] = bf_lo(v.z); o[5] = bf_hi(v.z); o[6] = bf_lo(v.w); o[7] = bf_hi(v.w);
    };
    float win[3][3][8];   // dy rows h - 1 + r, columns x - 1 + j
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        load(h + r - 1, -1, win[r][0]);
        load(h + r - 1, 0, win[r][1]);
    }
    for (int xx = 0; xx < W; ++xx) {
#pragma unroll
        for (int r = 0; r < 3; ++r) load(h + r - 1, xx + 1, win[r][2]);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = 0.f;
            // dx[h][x] = sum_{ky,kx} w[ky][kx] dy[h - ky + 1][x - kx + 1]
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) a = fmaf(w2p[(ky * 3 + kx) * C3 + c0 + e], win[2 - ky][2 - kx][e], a);
            o[e] = a;
        }
        u32x4 wv;
        wv.x = bf_pack(o[0], o[1]); wv.y = bf_pack(o[2], o[3]); wv.z = bf_pack(o[4], o[5]); wv.w = bf_pack(o[6], o[7]);
        *reinterpret_cast<u32x4*>(dx + (((int64_t)b * H + h) * W + xx) * C3 + c0) = wv;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                win[r][0][e] = win[r][1][e];
                win[r][1][e] = win[r][2][e];
            }
    }
}

__global__ __launch_bounds__(256) void dw_plain_bwd_w_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, float* __restrict__ wpart,
                                                             int B, int H, int W, int C3) {
    const int G = C3 / 8;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)B * H * G) return;
    const int gq = (int)(t % G);
    const int64_t bh = t / G;
    const int h = (int)(bh % H), b = (int)(bh / H);
    const int c0 = gq * 8;
    auto load = [&](const bf16_t* src, int yy, int xx, float* o) {
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.f;
            return;
        }
        const u32x4 v = *reinterpret_cast<const u32x4*>(src + (((int64_t)b * H + yy) * W + xx) * C3 + c0);
        o[0] = bf_lo(v.x); o[1] = bf_hi(v.x); o[2] = bf_lo(v.y); o[3] = bf_hi(v.y);
        o[4] = bf_lo(v.z); o[5] = bf_hi(v.z); o[6] = bf_lo(v.w); o[7] = bf_hi(v.w);
    };
    float win[3][3][8];   // input rows h - 1 + ky, columns x - 1 + kx
    float acc[10][8];
#pragma unroll
    for (int k = 0; k < 10; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        load(x, h + r - 1, -1, win[r][0]);
        load(x, h + r - 1, 0, win[r][1]);
    }
    for (int xx = 0; xx < W; ++xx) {
#pragma unroll
        for (int r = 0; r < 3; ++r) load(x, h + r - 1, xx + 1, win[r][2]);
        float d[8];
        load(dy, h, xx, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc[ky * 3 + kx][e] = fmaf(d[e], win[ky][kx][e], acc[ky * 3 + kx][e]);
            acc[9][e] += d[e];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                win[r][0][e] = win[r][1][e];
                win[r][1][e] = win[r][2][e];
            }
    }
    float* out = wpart + (((int64_t)b * H + h) * 10) * C3 + c0;
#pragma unroll
    for (int k = 0; k < 10; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) out[(int64_t)k * C3 + e] = acc[k][e];
}

// ---- per-(image, head) products -------------------------------------------------------------------------------------------
constexpr int GRAM_ROWS = 256;   // pixels per split (fixed: the splits of an image do not depend on the batch)
constexpr int GRAM_TILE = 32;
constexpr int CH_MAX = 96;       // channels per head of these two kernels (LDS of the apply kernel); wider heads: *_wide_bf16_kernel

// slab[z][split][i][j] = sum_{p in split} X[b][p][xo + h ch + i] * Y[b][p][yo + h ch + j],  z = b heads + h, grid (splits, B heads)
template <int MAXU>
__global__ __launch_bounds__(256) void gram_bf16_kernel(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ Y, int ldy,
                                                        float* __restrict__ slab, int P, int heads, int ch) {
    __shared__ float xs[GRAM_TILE][CH_MAX + 1];
    __shared__ float ys[GRAM_TILE][CH_MAX + 1];
    const int z = blockIdx.y, b = z / heads, h = z % heads, split = blockIdx.x, splits = gridDim.x;
    const int p0 = split * GRAM_ROWS, p1 = p0 + GRAM_ROWS < P ? p0 + GRAM_ROWS : P;
    const int nent = ch * ch, g8 = ch / 8;
    int ii[MAXU], jj[MAXU];
    float acc[MAXU];
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
        const int e = threadIdx.x + 256 * u;
        ii[u] = e < nent ? e / ch : 0;
        jj[u] = e < nent ? e % ch : 0;
        acc[u] = 0.f;
    }
    const bf16_t* xb = X + (int64_t)b * P * ldx + h * ch;
    const bf16_t* yb = Y + (int64_t)b * P * ldy + h * ch;
    for (int pt = p0; pt < p1; pt += GRAM_TILE) {
        for (int idx = threadIdx.x; idx < GRAM_TILE * g8 * 2; idx += 256) {
            const int which = idx / (GRAM_TILE * g8), rem = idx % (GRAM_TILE * g8);
            const int r = rem / g8, c = (rem % g8) * 8, p = pt + r;
            float(*dst)[CH_MAX + 1] = which ? ys : xs;
            if (p < p1) {
                const u32x4 v = which ? *reinterpret_cast<const u32x4*>(yb + (int64_t)p * ldy + c) : *reinterpret_cast<const u32x4*>(xb + (int64_t)p * ldx + c);
                dst[r][c + 0] = bf_lo(v.x); dst[r][c + 1] = bf_hi(v.x); dst[r][c + 2] = bf_lo(v.y); dst[r][c + 3] = bf_hi(v.y);
                dst[r][c + 4] = bf_lo(v.z); dst[r][c + 5] = bf_hi(v.z); dst[r][c + 6] = bf_lo(v.w); dst[r][c + 7] = bf_hi(v.w);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) dst[r][c + e] = 0.f;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < GRAM_TILE; ++r)
#pragma unroll
            for (int u = 0; u < MAXU; ++u) acc[u] = fmaf(xs[r][ii[u]], ys[r][jj[u]], acc[u]);
        __syncthreads();
    }
    float* out = slab + ((int64_t)z * splits + split) * nent;
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
        const int e = threadIdx.x + 256 * u;
        if (e < nent) out[e] = acc[u];
    }
}

int gram_splits(int P) { return cdiv(P, GRAM_ROWS); }

// ---- wide heads: CH_MAX < ch <= CH_WIDE (PromptIR's 704-channel noise_level3 block: 4 heads of 176) -----------------------
// The narrow kernels keep a whole ch x ch product per block (accumulators / LDS); these tile it instead.  Every output element is
// the same fp32 fmaf chain as in the narrow kernels (pixels resp. j in increasing order), so the numerics are those of the narrow path.
constexpr int CH_WIDE = 256;     // the fp32 softmax attention kernels' limit (restormer.hip SM_MAXU)
constexpr int WG_T = 64;         // gram: a 64 x 64 tile of G per block, 4 x 4 entries per thread (rows ty + 16 a, columns tx + 16 c)

// grid (splits, B heads, ceil(ch / 64)^2); slab layout as gram_bf16_kernel
__global__ __launch_bounds__(256) void gram_wide_bf16_kernel(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ Y, int ldy,
                                                             float* __restrict__ slab, int P, int heads, int ch) {
    __shared__ float xs[GRAM_TILE][WG_T];
    __shared__ float ys[GRAM_TILE][WG_T];
    const int z = blockIdx.y, b = z / heads, h = z % heads, split = blockIdx.x, splits = gridDim.x;
    const int nt = (ch + WG_T - 1) / WG_T;
    const int i0 = (int)(blockIdx.z / nt) * WG_T, j0 = (int)(blockIdx.z % nt) * WG_T;
    const int p0 = split * GRAM_ROWS, p1 = p0 + GRAM_ROWS < P ? p0 + GRAM_ROWS : P;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
    const bf16_t* xb = X + (int64_t)b * P * ldx + h * ch + i0;
    const bf16_t* yb = Y + (int64_t)b * P * ldy + h * ch + j0;
    for (int pt = p0; pt < p1; pt += GRAM_TILE) {
        // 2 maps x 32 pixels x 8 groups of 8 channels = 512 16-byte pieces, two per thread; outside the split / the head: zeros
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int idx = threadIdx.x + 256 * k;
            const int which = idx >> 8, r = (idx >> 3) & 31, c = (idx & 7) * 8, p = pt + r;
            float* d = which ? &ys[r][c] : &xs[r][c];
            if (p < p1 && (which ? j0 : i0) + c < ch) {
                const u32x4 v = which ? *reinterpret_cast<const u32x4*>(yb + (int64_t)p * ldy + c) : *reinterpret_cast<const u32x4*>(xb + (int64_t)p * ldx + c);
                d[0] = bf_lo(v.x); d[1] = bf_hi(v.x); d[2] = bf_lo(v.y); d[3] = bf_hi(v.y);
                d[4] = bf_lo(v.z); d[5] = bf_hi(v.z); d[6] = bf_lo(v.w); d[7] = bf_hi(v.w);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) d[e] = 0.f;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < GRAM_TILE; ++r) {
            float xv[4], yv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                xv[a] = xs[r][ty + 16 * a];
                yv[a] = ys[r][tx + 16 * a];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = fmaf(xv[a], yv[c], acc[a][c]);
        }
        __syncthreads();
    }
    float* out = slab + ((int64_t)z * splits + split) * ch * ch;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + ty + 16 * a;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx + 16 * c;
            if (i < ch && j < ch) out[(int64_t)i * ch + j] = acc[a][c];
        }
    }
}

int launch_gram(const bf16_t* X, int ldx, const bf16_t* Y, int ldy, float* slab, int B, int P, int heads, int ch, hipStream_t s) {
    if (ch > CH_MAX) {
        trace_tag("rst_bf16.gram_wide");
        const int nt = cdiv(ch, WG_T);
        gram_wide_bf16_kernel<<<dim3((unsigned)gram_splits(P), (unsigned)(B * heads), (unsigned)(nt * nt)), dim3(256), 0, s>>>(X, ldx, Y, ldy,
                                                                                                                                slab, P, heads, ch);
        DCPT_CHECK_LAUNCH("rst_bf16_gram_wide");
        return DCPT_OK;
    }
    trace_tag("rst_bf16.gram");
    const dim3 grid((unsigned)gram_splits(P), (unsigned)(B * heads)), blk(256);
    const int need = cdiv(ch * ch, 256);
    if (need <= 1) gram_bf16_kernel<1><<<grid, blk, 0, s>>>(X, ldx, Y, ldy, slab, P, heads, ch);
    else if (need <= 4) gram_bf16_kernel<4><<<grid, blk, 0, s>>>(X, ldx, Y, ldy, slab, P, heads, ch);
    else if (need <= 9) gram_bf16_kernel<9><<<grid, blk, 0, s>>>(X, ldx, Y, ldy, slab, P, heads, ch);
    else if (need <= 16) gram_bf16_kernel<16><<<grid, blk, 0, s>>>(X, ldx, Y, ldy, slab, P, heads, ch);
    else gram_bf16_kernel<36><<<grid, blk, 0, s>>>(X, ldx, Y, ldy, slab, P, heads, ch);
    DCPT_CHECK_LAUNCH("rst_bf16_gram");
    return DCPT_OK;
}

// O[b][p][oo + h ch + i] = sum_j A[z][i][j] V[b][p][vo + h ch + j]  (+ cs[b csb + h ch + i] R[b][p][h ch + i]),  grid (P / 32, B heads)
// dynamic LDS: A^T [ch][ch] + V tile [32][ch] (fp32); a thread computes 8 consecutive i of one pixel and stores 16 bytes
__global__ __launch_bounds__(256) void apply_bf16_kernel(const float* __restrict__ A, const bf16_t* __restrict__ V, int ldv,
                                                         const bf16_t* __restrict__ R, int ldr, const float* __restrict__ cs, int csb,
                                                         bf16_t* __restrict__ O, int ldo, int P, int heads, int ch) {
    extern __shared__ float sm[];
    float* at = sm;              // at[j * ch + i] = A[i][j]
    float* vs = sm + ch * ch;    // vs[r * ch + j]
    const int z = blockIdx.y, b = z / heads, h = z % heads;
    const int p0 = blockIdx.x * GRAM_TILE;
    const int g8 = ch / 8;
    const float* Az = A + (int64_t)z * ch * ch;
    for (int e = threadIdx.x; e < ch * ch; e += 256) {
        const int i = e / ch, j = e % ch;
        at[j * ch + i] = Az[e];
    }
    const bf16_t* vb = V + (int64_t)b * P * ldv + h * ch;
    for (int idx = threadIdx.x; idx < GRAM_TILE * g8; idx += 256) {
        const int r = idx / g8, c = (idx % g8) * 8, p = p0 + r;
        float* d = vs + r * ch + c;
        if (p < P) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(vb + (int64_t)p * ldv + c);
            d[0] = bf_lo(v.x); d[1] = bf_hi(v.x); d[2] = bf_lo(v.y); d[3] = bf_hi(v.y);
            d[4] = bf_lo(v.z); d[5] = bf_hi(v.z); d[6] = bf_lo(v.w); d[7] = bf_hi(v.w);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = 0.f;
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < GRAM_TILE * g8; idx += 256) {
        const int r = idx / g8, i0 = (idx % g8) * 8, p = p0 + r;
        if (p >= P) continue;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        const float* vr = vs + r * ch;
        for (int j = 0; j < ch; ++j) {
            const float v = vr[j];
            const float4 a0 = *reinterpret_cast<const float4*>(at + j * ch + i0);
            const float4 a1 = *reinterpret_cast<const float4*>(at + j * ch + i0 + 4);
            acc[0] = fmaf(a0.x, v, acc[0]); acc[1] = fmaf(a0.y, v, acc[1]); acc[2] = fmaf(a0.z, v, acc[2]); acc[3] = fmaf(a0.w, v, acc[3]);
            acc[4] = fmaf(a1.x, v, acc[4]); acc[5] = fmaf(a1.y, v, acc[5]); acc[6] = fmaf(a1.z, v, acc[6]); acc[7] = fmaf(a1.w, v, acc[7]);
        }
        const int64_t row = (int64_t)b * P + p;
        if (R) {
            const u32x4 rv = *reinterpret_cast<const u32x4*>(R + row * ldr + h * ch + i0);
            const float rr[8] = {bf_lo(rv.x), bf_hi(rv.x), bf_lo(rv.y), bf_hi(rv.y), bf_lo(rv.z), bf_hi(rv.z), bf_lo(rv.w), bf_hi(rv.w)};
            const float* c = cs + (int64_t)b * csb + h * ch + i0;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(c[e], rr[e], acc[e]);
        }
        u32x4 wv;
        wv.x = bf_pack(acc[0], acc[1]); wv.y = bf_pack(acc[2], acc[3]); wv.z = bf_pack(acc[4], acc[5]); wv.w = bf_pack(acc[6], acc[7]);
        *reinterpret_cast<u32x4*>(O + row * ldo + h * ch + i0) = wv;
    }
}

// wide heads: apply_bf16_kernel tiled over the output channels.  grid (P / 64, B heads, ch / 32); dynamic LDS: the fp32 A^T tile
// [ch][32] (A is never rounded) + the 64-pixel V tile [64][ch] kept in bf16 (widened on read, exact) = 256 ch bytes, 64 KiB at ch = 256:
// two blocks per CU.  A thread computes 8 consecutive i of one pixel (4 threads per pixel) and stores 16 bytes, like the narrow kernel.
constexpr int WA_IT = 32;   // output channels per block
constexpr int WA_PT = 64;   // pixels per block
__global__ __launch_bounds__(256) void apply_wide_bf16_kernel(const float* __restrict__ A, const bf16_t* __restrict__ V, int ldv,
                                                              const bf16_t* __restrict__ R, int ldr, const float* __restrict__ cs, int csb,
                                                              bf16_t* __restrict__ O, int ldo, int P, int heads, int ch) {
    extern __shared__ float sm[];
    float* at = sm;                                              // at[j * 32 + ii] = A[i0 + ii][j]
    bf16_t* vs = reinterpret_cast<bf16_t*>(sm + ch * WA_IT);    // vs[r * ch + j]
    const int z = blockIdx.y, b = z / heads, h = z % heads;
    const int p0 = blockIdx.x * WA_PT, i0 = blockIdx.z * WA_IT;
    const int g8 = ch / 8;
    const float* Az = A + (int64_t)z * ch * ch;
    for (int e = threadIdx.x; e < WA_IT * ch; e += 256) {
        const int j = e / WA_IT, ii = e % WA_IT, i = i0 + ii;
        at[e] = i < ch ? Az[(int64_t)i * ch + j] : 0.f;
    }
    const bf16_t* vb = V + (int64_t)b * P * ldv + h * ch;
    for (int idx = threadIdx.x; idx < WA_PT * g8; idx += 256) {
        const int r = idx / g8, c = (idx % g8) * 8, p = p0 + r;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (p < P) v = *reinterpret_cast<const u32x4*>(vb + (int64_t)p * ldv + c);
        *reinterpret_cast<u32x4*>(vs + r * ch + c) = v;
    }
    __syncthreads();
    const int r = threadIdx.x >> 2, ii0 = (threadIdx.x & 3) * 8, p = p0 + r, i = i0 + ii0;
    if (p >= P || i >= ch) return;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const uint32_t* vr = reinterpret_cast<const uint32_t*>(vs + r * ch);
    for (int j2 = 0; j2 < ch / 2; ++j2) {
        const uint32_t vv = vr[j2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float v = t ? bf_hi(vv) : bf_lo(vv);
            const float* arow = at + (2 * j2 + t) * WA_IT + ii0;
            const float4 a0 = *reinterpret_cast<const float4*>(arow);
            const float4 a1 = *reinterpret_cast<const float4*>(arow + 4);
            acc[0] = fmaf(a0.x, v, acc[0]); acc[1] = fmaf(a0.y, v, acc[1]); acc[2] = fmaf(a0.z, v, acc[2]); acc[3] = fmaf(a0.w, v, acc[3]);
            acc[4] = fmaf(a1.x, v, acc[4]); acc[5] = fmaf(a1.y, v, acc[5]); acc[6] = fmaf(a1.z, v, acc[6]); acc[7] = fmaf(a1.w, v, acc[7]);
        }
    }
    const int64_t row = (int64_t)b * P + p;
    if (R) {
        const u32x4 rv = *reinterpret_cast<const u32x4*>(R + row * ldr + h * ch + i);
        const float rr[8] = {bf_lo(rv.x), bf_hi(rv.x), bf_lo(rv.y), bf_hi(rv.y), bf_lo(rv.z), bf_hi(rv.z), bf_lo(rv.w), bf_hi(rv.w)};
        const float* c = cs + (int64_t)b * csb + h * ch + i;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(c[e], rr[e], acc[e]);
    }
    u32x4 wv;
    wv.x = bf_pack(acc[0], acc[1]); wv.y = bf_pack(acc[2], acc[3]); wv.z = bf_pack(acc[4], acc[5]); wv.w = bf_pack(acc[6], acc[7]);
    *reinterpret_cast<u32x4*>(O + row * ldo + h * ch + i) = wv;
}

int launch_apply(const float* A, const bf16_t* V, int ldv, const bf16_t* R, int ldr, const float* cs, int csb, bf16_t* O, int ldo, int B, int P,
                 int heads, int ch, hipStream_t s) {
    if (ch > CH_MAX) {
        trace_tag("rst_bf16.apply_wide");
        const size_t lds = (size_t)ch * WA_IT * sizeof(float) + (size_t)WA_PT * ch * sizeof(bf16_t);
        apply_wide_bf16_kernel<<<dim3((unsigned)cdiv(P, WA_PT), (unsigned)(B * heads), (unsigned)cdiv(ch, WA_IT)), dim3(256), lds, s>>>(
            A, V, ldv, R, ldr, cs, csb, O, ldo, P, heads, ch);
        DCPT_CHECK_LAUNCH("rst_bf16_apply_wide");
        return DCPT_OK;
    }
    trace_tag("rst_bf16.apply");
    const size_t lds = (size_t)(ch * ch + GRAM_TILE * ch) * sizeof(float);
    apply_bf16_kernel<<<dim3((unsigned)cdiv(P, GRAM_TILE), (unsigned)(B * heads)), dim3(256), lds, s>>>(A, V, ldv, R, ldr, cs, csb, O, ldo, P, heads, ch);
    DCPT_CHECK_LAUNCH("rst_bf16_apply");
    return DCPT_OK;
}

// ---- weights --------------------------------------------------------------------------------------------------------------
// bf16 operand image of an fp32 [N][K] weight (transpose: [K][N]) through an fp32 staging buffer of N K floats
int pack_bf16(const float* w, float* stage, bf16_t* out, int N, int K, bool transpose, hipStream_t s) {
    const float* src = w;
    if (transpose) {
        DCPT_TRY(launch_wpack(w, stage, nullptr, N, K, WP_TRANSPOSE, s));
        src = stage;
    }
    return launch_cast_f32_bf16(src, out, (int64_t)N * K, s);
}

int nt(const bf16_t* A, int lda, const bf16_t* Bw, int N, int K, bf16_t* C, int ldc, int64_t M, const bf16_t* res, hipStream_t s) {
    GemmNTB g = gemm_ntb_linear(A, lda, M, K, Bw, N, C, ldc);
    g.res = res;
    return launch_gemm_nt_bf16(g, res ? EB_RESID : EB_PLAIN, s);
}

// ---- MDTA workspace --------------------------------------------------------------------------------------------------------
struct MdtaWsB {
    bf16_t *wq, *wp;              // [3C][C], [C][C] forward operands; backward: their transposes [C][3C], [C][C]
    float* stage;                 // [3C][C] fp32 staging of the transposes
    float* w2p;                   // [9][3C]
    float* sqpart;                // [B][H][2C]
    float* gslab;                 // [B heads][splits][ch][ch]
    bf16_t *r_xn, *r_qkv1, *r_out;   // lean / balanced: what the caller did not keep
    float* stats;                 // [2M] statistics of a recomputed LayerNorm
    bf16_t *d_att, *dqkv, *dqkv1, *dxn;
    float *dG, *dGT, *scr, *cqk, *dtpart, *scr2;
    float *slab, *wpart, *lnpart;
    int splits, nblk_dwb;
};

bool mdta_shape_ok(int B, int H, int W, int C, int heads) {
    return B > 0 && H > 0 && W > 0 && heads > 0 && C % heads == 0 && (C / heads) % 8 == 0 && C / heads <= CH_WIDE && C <= 1024;
}

// kept: the caller supplies xn, qkv1 and out_att (full save mode), so their workspace copies are not reserved
size_t mdta_layout(int B, int H, int W, int c, int heads, int backward, bool kept, void* base, size_t bytes, MdtaWsB* out) {
    WsAlloc a(base, bytes);
    MdtaWsB w{};
    const int64_t M = (int64_t)B * H * W;
    const int P = H * W, ch = c / heads;
    w.splits = gram_splits(P);
    w.wq = a.get<bf16_t>((size_t)3 * c * c);
    w.wp = a.get<bf16_t>((size_t)c * c);
    w.w2p = a.get<float>((size_t)27 * c);
    w.gslab = a.get<float>((size_t)B * heads * w.splits * ch * ch);
    if (!kept) {
        w.r_xn = a.get<bf16_t>((size_t)M * c);
        w.r_qkv1 = a.get<bf16_t>((size_t)M * 3 * c);
        w.r_out = a.get<bf16_t>((size_t)M * c);
    }
    if (!backward) {
        w.sqpart = a.get<float>((size_t)B * H * 2 * c);
    } else {
        w.stage = a.get<float>((size_t)3 * c * c);
        w.stats = a.get<float>((size_t)2 * M);
        w.d_att = a.get<bf16_t>((size_t)M * c);
        w.dqkv = a.get<bf16_t>((size_t)M * 3 * c);
        w.dqkv1 = a.get<bf16_t>((size_t)M * 3 * c);
        w.dxn = a.get<bf16_t>((size_t)M * c);
        w.dG = a.get<float>((size_t)B * heads * ch * ch);
        w.dGT = a.get<float>((size_t)B * heads * ch * ch);
        w.scr = a.get<float>((size_t)B * heads * ch * ch);
        w.cqk = a.get<float>((size_t)B * 2 * c);
        w.dtpart = a.get<float>((size_t)B * heads);
        w.scr2 = a.get<float>((size_t)3 * c);
        size_t sl = 0;   // qkv and project_out share the slabs
        wgrad_need_bf16(M, 3 * c, c, &sl, nullptr);
        wgrad_need_bf16(M, c, c, &sl, nullptr);
        w.slab = a.get<float>(sl);
        w.nblk_dwb = H;   // tap-gradient partials per image row
        w.wpart = a.get<float>((size_t)B * w.nblk_dwb * 10 * 3 * c);
        w.lnpart = a.get<float>((size_t)ln_bwd_waves(M) * 2 * c);
    }
    if (out) *out = w;
    return a.off;
}

// ---- GDFN workspace --------------------------------------------------------------------------------------------------------
struct GdfnWsB {
    bf16_t *w_in, *w_out;         // forward [2hp][C], [C][hp];  backward: transposes [C][2hp], [hp][C]
    float* stage;                 // fp32 staging of the packs (2 hp max(C, 9) floats) and the padded gradients
    float* w2p;                   // [9][2hp]
    bf16_t *r_xn, *r_t;
    float* stats;
    bf16_t *dt, *du, *dxn;
    float *slab, *wpart, *lnpart, *gpad;
    int nblk_dwb;
};

int gdfn_hp(int hidden) { return (hidden + 7) / 8 * 8; }

// kept: the caller supplies xn and t (full save mode)
size_t gdfn_layout(int B, int H, int W, int c, int hp, int backward, bool kept, void* base, size_t bytes, GdfnWsB* out) {
    WsAlloc a(base, bytes);
    GdfnWsB w{};
    const int64_t M = (int64_t)B * H * W;
    w.w_in = a.get<bf16_t>((size_t)2 * hp * c);
    w.w_out = a.get<bf16_t>((size_t)c * hp);
    w.stage = a.get<float>((size_t)2 * hp * (c > 9 ? c : 9));
    w.w2p = a.get<float>((size_t)18 * hp);
    if (!kept) {
        w.r_xn = a.get<bf16_t>((size_t)M * c);
        w.r_t = a.get<bf16_t>((size_t)M * hp);
    }
    if (backward) {
        w.stats = a.get<float>((size_t)2 * M);
        w.dt = a.get<bf16_t>((size_t)M * hp);
        w.du = a.get<bf16_t>((size_t)M * 2 * hp);
        w.dxn = a.get<bf16_t>((size_t)M * c);
        size_t sl = 0;   // project_in and project_out share the slabs
        wgrad_need_bf16(M, 2 * hp, c, &sl, nullptr);
        wgrad_need_bf16(M, c, hp, &sl, nullptr);
        w.slab = a.get<float>(sl);
        w.nblk_dwb = dw_ring_bwd_num_blocks_per_image(DwGeom{B, H, W, hp});
        w.wpart = a.get<float>((size_t)B * w.nblk_dwb * 10 * 2 * hp);
        w.lnpart = a.get<float>((size_t)ln_bwd_waves(M) * 2 * c);
        w.gpad = a.get<float>((size_t)2 * hp * (c > 9 ? c : 9) + (size_t)c * hp);
    }
    if (out) *out = w;
    return a.off;
}

bool gdfn_shape_ok(int B, int H, int W, int C, int hidden) {
    return B > 0 && H > 0 && W > 0 && hidden > 0 && C % 8 == 0 && C <= 1024 && dw_ring_usable(DwGeom{B, H, W, gdfn_hp(hidden)}, 2) &&
           dw_ring_bwd_usable(DwGeom{B, H, W, gdfn_hp(hidden)}, 2);
}

}  // namespace

// =====================================================================================================
extern "C" size_t dcpt_mdta_bf16_ws_bytes(int B, int H, int W, int C, int heads, int backward) {
    if (!mdta_shape_ok(B, H, W, C, heads)) return 0;
    return mdta_layout(B, H, W, C, heads, backward & 1, (backward & 2) != 0, nullptr, 0, nullptr);
}

extern "C" int dcpt_mdta_bf16_fwd(const dcpt_mdta_params* p, const uint16_t* x, uint16_t* y, const dcpt_mdta_saved_bf16* sv, void* ws,
                                  size_t ws_bytes, int B, int H, int W, int C, int heads, int flags, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && x && y && sv && p->norm_w && p->qkv_w && p->dw_w && p->proj_w && p->temperature && sv->mu && sv->rstd && sv->qkv &&
                       sv->nrm && sv->ghat && sv->attn && sv->attnT,
                   "mdta_bf16_fwd: null argument");
    DCPT_CHECK_ARG(mdta_shape_ok(B, H, W, C, heads),
                   "mdta_bf16_fwd: C=%d heads=%d (C %% heads == 0, C / heads a multiple of 8 and <= %d, C <= 1024)", C, heads, CH_WIDE);
    const bool biasfree = flags & DCPT_LN_BIASFREE;
    DCPT_CHECK_ARG(biasfree || p->norm_b, "mdta_bf16_fwd: WithBias LayerNorm needs norm_b");
    const float ln_eps = (flags & DCPT_LN_EPS_1E5) ? 1e-5f : 1e-6f;
    const bool softmax = (flags & DCPT_ATTN_SOFTMAX) != 0;
    MdtaWsB w;
    const size_t need = mdta_layout(B, H, W, C, heads, 0, sv->xn && sv->qkv1 && sv->out_att, ws, ws_bytes, &w);
    DCPT_CHECK_WS("mdta_bf16_fwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    const int P = H * W, ch = C / heads, C3 = 3 * C;
    const bf16_t* xb = reinterpret_cast<const bf16_t*>(x);
    bf16_t* xn = sv->xn ? reinterpret_cast<bf16_t*>(sv->xn) : w.r_xn;
    bf16_t* qkv1 = sv->qkv1 ? reinterpret_cast<bf16_t*>(sv->qkv1) : w.r_qkv1;
    bf16_t* qkv = reinterpret_cast<bf16_t*>(sv->qkv);
    bf16_t* out_att = sv->out_att ? reinterpret_cast<bf16_t*>(sv->out_att) : w.r_out;
    DCPT_TRY(pack_bf16(p->qkv_w, nullptr, w.wq, C3, C, false, s));
    DCPT_TRY(pack_bf16(p->proj_w, nullptr, w.wp, C, C, false, s));
    DCPT_TRY(launch_dw_pack_weights(p->dw_w, w.w2p, C3, s));
    DCPT_TRY(launch_ln_fwd_rows(xb, p->norm_w, p->norm_b, xn, sv->mu, sv->rstd, M, C, ln_eps, biasfree, s));
    DCPT_TRY(nt(xn, C, w.wq, C3, C, qkv1, C3, M, nullptr, s));
    trace_tag("rst_bf16.dw_sq_fwd");
    dw_sq_fwd_kernel<<<dim3((unsigned)cdiv64((int64_t)B * H * (C3 / 8), 256)), dim3(256), 0, s>>>(qkv1, w.w2p, qkv, w.sqpart, B, H, W, C3, 2 * C);
    DCPT_CHECK_LAUNCH("rst_bf16_dw_sq_fwd");
    DCPT_TRY(launch_mdta_sq_norm(w.sqpart, H, sv->nrm, B, 2 * C, s));
    DCPT_TRY(launch_gram(qkv, C3, qkv + C, C3, w.gslab, B, P, heads, ch, s));
    DCPT_TRY(launch_mdta_attn_finalize(w.gslab, w.splits, sv->nrm, p->temperature, sv->ghat, sv->attn, sv->attnT, B, heads, ch, C, softmax, s));
    DCPT_TRY(launch_apply(sv->attn, qkv + 2 * C, C3, nullptr, 0, nullptr, 0, out_att, C, B, P, heads, ch, s));
    return nt(out_att, C, w.wp, C, C, reinterpret_cast<bf16_t*>(y), C, M, xb, s);
}

extern "C" int dcpt_mdta_bf16_bwd(const dcpt_mdta_params* p, const dcpt_mdta_params_grads* gr, const uint16_t* x, const dcpt_mdta_saved_bf16* sv,
                                  const uint16_t* dy, uint16_t* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int heads, int flags,
                                  dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && gr && x && sv && dy && dx && p->norm_w && p->qkv_w && p->dw_w && p->proj_w && p->temperature && sv->mu && sv->rstd &&
                       sv->qkv && sv->nrm && sv->ghat && sv->attn && sv->attnT && gr->norm_w && gr->qkv_w && gr->dw_w && gr->proj_w &&
                       gr->temperature,
                   "mdta_bf16_bwd: null argument");
    DCPT_CHECK_ARG(mdta_shape_ok(B, H, W, C, heads),
                   "mdta_bf16_bwd: C=%d heads=%d (C %% heads == 0, C / heads a multiple of 8 and <= %d, C <= 1024)", C, heads, CH_WIDE);
    const bool biasfree = flags & DCPT_LN_BIASFREE;
    DCPT_CHECK_ARG(biasfree || (p->norm_b && gr->norm_b), "mdta_bf16_bwd: WithBias LayerNorm needs norm_b and its gradient");
    const float ln_eps = (flags & DCPT_LN_EPS_1E5) ? 1e-5f : 1e-6f;
    const bool softmax = (flags & DCPT_ATTN_SOFTMAX) != 0;
    MdtaWsB w;
    const size_t need = mdta_layout(B, H, W, C, heads, 1, sv->xn && sv->qkv1 && sv->out_att, ws, ws_bytes, &w);
    DCPT_CHECK_WS("mdta_bf16_bwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    const int P = H * W, ch = C / heads, C3 = 3 * C;
    const bf16_t* xb = reinterpret_cast<const bf16_t*>(x);
    const bf16_t* dyb = reinterpret_cast<const bf16_t*>(dy);
    const bf16_t* qkv = reinterpret_cast<const bf16_t*>(sv->qkv);
    const bf16_t* xn = reinterpret_cast<const bf16_t*>(sv->xn);
    const bf16_t* qkv1 = reinterpret_cast<const bf16_t*>(sv->qkv1);
    const bf16_t* out_att = reinterpret_cast<const bf16_t*>(sv->out_att);
    // what the forward pass did not keep: LN(x) (statistics to scratch: the saved ones are identical), the qkv conv, attn @ v
    if (!xn) {
        DCPT_TRY(launch_ln_fwd_rows(xb, p->norm_w, p->norm_b, w.r_xn, w.stats, w.stats + M, M, C, ln_eps, biasfree, s));
        xn = w.r_xn;
    }
    if (!qkv1) {
        DCPT_TRY(pack_bf16(p->qkv_w, nullptr, w.wq, C3, C, false, s));
        DCPT_TRY(nt(xn, C, w.wq, C3, C, w.r_qkv1, C3, M, nullptr, s));
        qkv1 = w.r_qkv1;
    }
    if (!out_att) {
        DCPT_TRY(launch_apply(sv->attn, qkv + 2 * C, C3, nullptr, 0, nullptr, 0, w.r_out, C, B, P, heads, ch, s));
        out_att = w.r_out;
    }
    // d_att = dy Wproj ; dWproj = dy^T out_att
    DCPT_TRY(pack_bf16(p->proj_w, w.stage, w.wp, C, C, true, s));
    DCPT_TRY(nt(dyb, C, w.wp, C, C, w.d_att, C, M, nullptr, s));
    DCPT_TRY(launch_wgrad_bf16(GemmTNB{}, dyb, C, C, out_att, C, C, M, w.slab, nullptr, gr->proj_w, nullptr, WR_PLAIN, s));
    // dattn = d_att^T v (per image and head);  dv = d_att attn  (attn^T as the applied matrix)
    DCPT_TRY(launch_gram(w.d_att, C, qkv + 2 * C, C3, w.gslab, B, P, heads, ch, s));
    DCPT_TRY(launch_apply(sv->attnT, w.d_att, C, nullptr, 0, nullptr, 0, w.dqkv + 2 * C, C3, B, P, heads, ch, s));
    // through ReLU / softmax, temperature and the normalisation
    DCPT_TRY(launch_mdta_attn_bwd(w.gslab, w.splits, sv->attn, sv->ghat, sv->nrm, p->temperature, w.dG, w.dGT, w.cqk, w.dtpart, w.scr, B, heads, ch,
                                  C, softmax, s));
    DCPT_TRY(launch_mdta_dtemp_reduce(w.dtpart, gr->temperature, B, heads, s));
    // dq = dG k + cq q ;  dk = dG^T q + ck k
    DCPT_TRY(launch_apply(w.dG, qkv + C, C3, qkv, C3, w.cqk, 2 * C, w.dqkv, C3, B, P, heads, ch, s));
    DCPT_TRY(launch_apply(w.dGT, qkv, C3, qkv + C, C3, w.cqk + C, 2 * C, w.dqkv + C, C3, B, P, heads, ch, s));
    // depthwise backward on the ring
    DCPT_TRY(launch_dw_pack_weights(p->dw_w, w.w2p, C3, s));
    trace_tag("rst_bf16.dw_plain_bwd");
    {
        const dim3 grid((unsigned)cdiv64((int64_t)B * H * (C3 / 8), 256)), blk(256);
        dw_plain_bwd_dx_kernel<<<grid, blk, 0, s>>>(w.dqkv, w.w2p, w.dqkv1, B, H, W, C3);
        DCPT_CHECK_LAUNCH("rst_bf16_dw_plain_bwd_dx");
        dw_plain_bwd_w_kernel<<<grid, blk, 0, s>>>(w.dqkv, qkv1, w.wpart, B, H, W, C3);
        DCPT_CHECK_LAUNCH("rst_bf16_dw_plain_bwd_w");
    }
    DCPT_TRY(launch_dw_wgrad_reduce(w.wpart, B * w.nblk_dwb, C3, gr->dw_w, w.scr2, s));
    // qkv 1x1
    DCPT_TRY(pack_bf16(p->qkv_w, w.stage, w.wq, C3, C, true, s));
    DCPT_TRY(nt(w.dqkv1, C3, w.wq, C, C3, w.dxn, C, M, nullptr, s));
    DCPT_TRY(launch_wgrad_bf16(GemmTNB{}, w.dqkv1, C3, C3, xn, C, C, M, w.slab, nullptr, gr->qkv_w, nullptr, WR_PLAIN, s));
    // dx = dy + LN-backward
    DCPT_TRY(launch_ln_bwd_rows(w.dxn, xb, sv->mu, sv->rstd, p->norm_w, dyb, reinterpret_cast<bf16_t*>(dx), w.lnpart, M, C, biasfree, s));
    return launch_colpart_reduce(w.lnpart, ln_bwd_waves(M), 2, C, gr->norm_w, biasfree ? nullptr : gr->norm_b, nullptr, s);
}

// =====================================================================================================
extern "C" size_t dcpt_gdfn_bf16_ws_bytes(int B, int H, int W, int C, int hidden, int backward) {
    if (!gdfn_shape_ok(B, H, W, C, hidden)) return 0;
    return gdfn_layout(B, H, W, C, gdfn_hp(hidden), backward & 1, (backward & 2) != 0, nullptr, 0, nullptr);
}

extern "C" int dcpt_gdfn_bf16_fwd(const dcpt_gdfn_params* p, const uint16_t* x, uint16_t* y, const dcpt_gdfn_saved_bf16* sv, void* ws,
                                  size_t ws_bytes, int B, int H, int W, int C, int hidden, int flags, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && x && y && sv && p->norm_w && p->in_w && p->dw_w && p->out_w && sv->mu && sv->rstd && sv->u, "gdfn_bf16_fwd: null argument");
    DCPT_CHECK_ARG(gdfn_shape_ok(B, H, W, C, hidden), "gdfn_bf16_fwd: C=%d hidden=%d (C %% 8 == 0, hidden > 0; bf16 depthwise ring usable)", C, hidden);
    const bool biasfree = flags & DCPT_LN_BIASFREE;
    DCPT_CHECK_ARG(biasfree || p->norm_b, "gdfn_bf16_fwd: WithBias LayerNorm needs norm_b");
    const float ln_eps = (flags & DCPT_LN_EPS_1E5) ? 1e-5f : 1e-6f;
    const int hp = gdfn_hp(hidden);
    GdfnWsB w;
    const size_t need = gdfn_layout(B, H, W, C, hp, 0, sv->xn && sv->t, ws, ws_bytes, &w);
    DCPT_CHECK_WS("gdfn_bf16_fwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    const bf16_t* xb = reinterpret_cast<const bf16_t*>(x);
    bf16_t* xn = sv->xn ? reinterpret_cast<bf16_t*>(sv->xn) : w.r_xn;
    bf16_t* tg = sv->t ? reinterpret_cast<bf16_t*>(sv->t) : w.r_t;
    bf16_t* u = reinterpret_cast<bf16_t*>(sv->u);
    DCPT_TRY(launch_gdfn_pack(p->in_w, w.stage, C, hidden, hp, 0, s));
    DCPT_TRY(launch_cast_f32_bf16(w.stage, w.w_in, (int64_t)2 * hp * C, s));
    DCPT_TRY(launch_gdfn_pack(p->out_w, w.stage, C, hidden, hp, 2, s));
    DCPT_TRY(launch_cast_f32_bf16(w.stage, w.w_out, (int64_t)C * hp, s));
    DCPT_TRY(launch_gdfn_pack(p->dw_w, w.w2p, C, hidden, hp, 1, s));
    DCPT_TRY(launch_ln_fwd_rows(xb, p->norm_w, p->norm_b, xn, sv->mu, sv->rstd, M, C, ln_eps, biasfree, s));
    DCPT_TRY(nt(xn, C, w.w_in, 2 * hp, C, u, 2 * hp, M, nullptr, s));
    DCPT_TRY(launch_dw_ring_gelu_fwd_bf16(u, w.w2p, tg, B, H, W, hp, s));
    return nt(tg, hp, w.w_out, C, hp, reinterpret_cast<bf16_t*>(y), C, M, xb, s);
}

extern "C" int dcpt_gdfn_bf16_bwd(const dcpt_gdfn_params* p, const dcpt_gdfn_params_grads* gr, const uint16_t* x, const dcpt_gdfn_saved_bf16* sv,
                                  const uint16_t* dy, uint16_t* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int hidden, int flags,
                                  dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && gr && x && sv && dy && dx && p->norm_w && p->in_w && p->dw_w && p->out_w && sv->mu && sv->rstd && sv->u && gr->norm_w &&
                       gr->in_w && gr->dw_w && gr->out_w,
                   "gdfn_bf16_bwd: null argument");
    DCPT_CHECK_ARG(gdfn_shape_ok(B, H, W, C, hidden), "gdfn_bf16_bwd: C=%d hidden=%d (C %% 8 == 0, hidden > 0; bf16 depthwise ring usable)", C, hidden);
    const bool biasfree = flags & DCPT_LN_BIASFREE;
    DCPT_CHECK_ARG(biasfree || (p->norm_b && gr->norm_b), "gdfn_bf16_bwd: WithBias LayerNorm needs norm_b and its gradient");
    const float ln_eps = (flags & DCPT_LN_EPS_1E5) ? 1e-5f : 1e-6f;
    const int hp = gdfn_hp(hidden);
    GdfnWsB w;
    const size_t need = gdfn_layout(B, H, W, C, hp, 1, sv->xn && sv->t, ws, ws_bytes, &w);
    DCPT_CHECK_WS("gdfn_bf16_bwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    const bf16_t* xb = reinterpret_cast<const bf16_t*>(x);
    const bf16_t* dyb = reinterpret_cast<const bf16_t*>(dy);
    const bf16_t* u = reinterpret_cast<const bf16_t*>(sv->u);
    const bf16_t* xn = reinterpret_cast<const bf16_t*>(sv->xn);
    const bf16_t* tg = reinterpret_cast<const bf16_t*>(sv->t);
    float* g_in = w.gpad;                                        // [2hp][C] (also [2hp][9])
    float* g_out = w.gpad + (size_t)2 * hp * (C > 9 ? C : 9);    // [C][hp]
    DCPT_TRY(launch_gdfn_pack(p->dw_w, w.w2p, C, hidden, hp, 1, s));
    if (!xn) {
        DCPT_TRY(launch_ln_fwd_rows(xb, p->norm_w, p->norm_b, w.r_xn, w.stats, w.stats + M, M, C, ln_eps, biasfree, s));
        xn = w.r_xn;
    }
    if (!tg) {
        DCPT_TRY(launch_dw_ring_gelu_fwd_bf16(u, w.w2p, w.r_t, B, H, W, hp, s));
        tg = w.r_t;
    }
    // dt = dy Wout ; dWout = dy^T t
    DCPT_TRY(launch_gdfn_pack(p->out_w, w.stage, C, hidden, hp, 3, s));
    DCPT_TRY(launch_cast_f32_bf16(w.stage, w.w_out, (int64_t)hp * C, s));
    DCPT_TRY(nt(dyb, C, w.w_out, hp, C, w.dt, hp, M, nullptr, s));
    DCPT_TRY(launch_wgrad_bf16(GemmTNB{}, dyb, C, C, tg, hp, hp, M, w.slab, nullptr, g_out, nullptr, WR_PLAIN, s));
    DCPT_TRY(launch_gdfn_unpack(g_out, gr->out_w, C, hidden, hp, 2, s));
    // gate + depthwise backward in one pass on the ring
    DCPT_TRY(launch_dw_ring_bwd_gelu_bf16(w.dt, u, w.w2p, w.du, w.wpart, B, H, W, hp, s));
    DCPT_TRY(launch_dw_wgrad_reduce(w.wpart, B * w.nblk_dwb, 2 * hp, g_in, g_out /*sink of the (absent) bias gradient*/, s));
    DCPT_TRY(launch_gdfn_unpack(g_in, gr->dw_w, C, hidden, hp, 1, s));
    // project_in
    DCPT_TRY(launch_gdfn_pack(p->in_w, w.stage, C, hidden, hp, 4, s));
    DCPT_TRY(launch_cast_f32_bf16(w.stage, w.w_in, (int64_t)C * 2 * hp, s));
    DCPT_TRY(nt(w.du, 2 * hp, w.w_in, C, 2 * hp, w.dxn, C, M, nullptr, s));
    DCPT_TRY(launch_wgrad_bf16(GemmTNB{}, w.du, 2 * hp, 2 * hp, xn, C, C, M, w.slab, nullptr, g_in, nullptr, WR_PLAIN, s));
    DCPT_TRY(launch_gdfn_unpack(g_in, gr->in_w, C, hidden, hp, 0, s));
    DCPT_TRY(launch_ln_bwd_rows(w.dxn, xb, sv->mu, sv->rstd, p->norm_w, dyb, reinterpret_cast<bf16_t*>(dx), w.lnpart, M, C, biasfree, s));
    return launch_colpart_reduce(w.lnpart, ln_bwd_waves(M), 2, C, gr->norm_w, biasfree ? nullptr : gr->norm_b, nullptr, s);
}

// =====================================================================================================
// glue between the blocks, bf16: NHWC pixel (un)shuffle and channel concat / split (restormer.hip's address maps, 2-byte elements)
namespace {
__global__ void pixel_shuffle_bf16_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int B, int Hc, int Wc, int C, int dir) {
    const int64_t total = (int64_t)B * Hc * Wc * 4 * C;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int cc = (int)(e % (4 * C));
        int64_t t = e / (4 * C);
        const int w = (int)(t % Wc);
        t /= Wc;
        const int h = (int)(t % Hc);
        const int64_t b = t / Hc;
        const int k = cc >> 2, ij = cc & 3;
        const int64_t fine = ((b * (2 * Hc) + 2 * h + (ij >> 1)) * (int64_t)(2 * Wc) + 2 * w + (ij & 1)) * C + k;
        if (dir == 0) out[e] = in[fine];
        else out[fine] = in[e];
    }
}

// 8-element (16-byte) pieces: Ca, Cb multiples of 8
__global__ void concat_bf16_kernel(bf16_t* __restrict__ a, bf16_t* __restrict__ b, bf16_t* __restrict__ cat, int64_t M, int Ca, int Cb, int dir) {
    const int qa = Ca / 8, qb = Cb / 8, qt = qa + qb;
    const int64_t total = M * qt;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(e % qt);
        const int64_t m = e / qt;
        u32x4* src = reinterpret_cast<u32x4*>((q < qa) ? a + m * Ca + 8 * q : b + m * Cb + 8 * (q - qa));
        u32x4* dst = reinterpret_cast<u32x4*>(cat + m * (int64_t)(Ca + Cb) + 8 * q);
        if (dir == 0) *dst = *src;
        else *src = *dst;
    }
}
}  // namespace

extern "C" int dcpt_pixel_unshuffle_bf16(const uint16_t* x, uint16_t* y, int B, int H, int W, int C, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0, "pixel_unshuffle_bf16: bad argument");
    trace_tag("rst_bf16.pixel_shuffle");
    pixel_shuffle_bf16_kernel<<<dim3(ew_grid((int64_t)B * H * W * C)), dim3(256), 0, (hipStream_t)stream>>>(x, y, B, H / 2, W / 2, C, 0);
    DCPT_CHECK_LAUNCH("pixel_unshuffle_bf16");
    return DCPT_OK;
}

extern "C" int dcpt_pixel_shuffle_bf16(const uint16_t* x, uint16_t* y, int B, int H, int W, int C4, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && C4 > 0 && C4 % 4 == 0, "pixel_shuffle_bf16: bad argument");
    trace_tag("rst_bf16.pixel_shuffle");
    pixel_shuffle_bf16_kernel<<<dim3(ew_grid((int64_t)B * H * W * C4)), dim3(256), 0, (hipStream_t)stream>>>(x, y, B, H, W, C4 / 4, 1);
    DCPT_CHECK_LAUNCH("pixel_shuffle_bf16");
    return DCPT_OK;
}

extern "C" int dcpt_concat_channels_bf16(const uint16_t* a, const uint16_t* b, uint16_t* out, int64_t M, int Ca, int Cb, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(a && b && out && M > 0 && Ca > 0 && Cb > 0 && Ca % 8 == 0 && Cb % 8 == 0, "concat_channels_bf16: bad argument (channels %% 8)");
    trace_tag("rst_bf16.concat");
    concat_bf16_kernel<<<dim3(ew_grid(M * ((Ca + Cb) / 8))), dim3(256), 0, (hipStream_t)stream>>>((bf16_t*)a, (bf16_t*)b, out, M, Ca, Cb, 0);
    DCPT_CHECK_LAUNCH("concat_channels_bf16");
    return DCPT_OK;
}

extern "C" int dcpt_split_channels_bf16(const uint16_t* cat, uint16_t* a, uint16_t* b, int64_t M, int Ca, int Cb, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(a && b && cat && M > 0 && Ca > 0 && Cb > 0 && Ca % 8 == 0 && Cb % 8 == 0, "split_channels_bf16: bad argument (channels %% 8)");
    trace_tag("rst_bf16.concat");
    concat_bf16_kernel<<<dim3(ew_grid(M * ((Ca + Cb) / 8))), dim3(256), 0, (hipStream_t)stream>>>(a, b, (bf16_t*)cat, M, Ca, Cb, 1);
    DCPT_CHECK_LAUNCH("split_channels_bf16");
    return DCPT_OK;
}
