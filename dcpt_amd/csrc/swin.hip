// SwinIR blocks (reference basicsr/archs/swinir_arch.py, the DCPT variant: no relative-position bias, no shift mask):
//   attention half  y = x + proj(WMSA_shift(qkv(LN1(x))))     dcpt_swin_attn_fwd/bwd
//   MLP half        y = x + fc2(gelu(fc1(LN2(x))))            dcpt_swin_mlp_fwd/bwd
//   RSTB conv       y = res + conv3x3(x) + bias (NHWC -> NHWC) dcpt_conv3x3_res_fwd/bwd
//   image affine    (x - mean) * r  and  x / r + mean         dcpt_img_affine
//
// Tokens stay in plain NHWC rows [M][C] throughout.  The cyclic shift (torch.roll by -shift), window partition, window
// reverse and the inverse roll are address arithmetic of the window kernel: token (i, j) of window (wy, wx) of image b is pixel
// ((wy*ws + i + shift) mod H, (wx*ws + j + shift) mod W), read from and written back to that pixel.  Windows at the image edge
// wrap around with no mask, as in the reference.
//
// Window kernel: one workgroup (4 waves) per (window, head).  Q (pre-scaled by head_dim^-0.5, as the reference scales q before
// the product), K and V of the <= 64 tokens go to LDS; S = Q K^T is up to four 32 x 32 tiles of v_mfma_f32_32x32x2_f32, one per
// wave; the row softmax runs in fp32 with max subtraction, one wave per row; O = P V is up to four more tiles.  The backward
// recomputes P from the saved per-row log-sum-exp and forms dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(dO O)),
// dQ = scale dS K, dK = dS^T (scale Q); every token belongs to one window per block, so d(qkv) is written without atomics.
#include "gemm.h"
#include "kernels.h"
#include "prof.h"
#include "swin_win.h"
#include "../../include/dcpt_hip.h"

namespace {

constexpr float SWIN_LN_EPS = 1e-5f;   // nn.LayerNorm default
constexpr int SP = WT + 1;             // LDS row stride of the token x token tiles (WT, WinGeom, win_token_row: swin_win.h)

// one 32 x 32 fp32 MFMA tile: acc += sum_{k < K} A(i, k) B(k, j); A(i, k) = a[i * sa_i + k * sa_k], B(k, j) = b[k * sb_k + j * sb_j]
// (LDS pointers already offset to the tile); K even
__device__ __forceinline__ floatx16 mfma_tile(const float* a, int sa_i, int sa_k, const float* b, int sb_k, int sb_j, int K, int lane) {
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int li = lane & 31, lk = lane >> 5;
    const float* pa = a + li * sa_i + lk * sa_k;
    const float* pb = b + lk * sb_k + li * sb_j;
    for (int k = 0; k < K; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k * sa_k], pb[k * sb_k], acc, 0, 0, 0);
    return acc;
}
// C/D map of the 32x32 MFMA: register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// load the head slice s (0 q, 1 k, 2 v) of the window's tokens into dst[WT][DP + 1] (zero padded to NP x DP), times mul
template <int DP>
__device__ __forceinline__ void load_slice(const float* __restrict__ src, int ld, int col0, const int64_t* rows, const WinGeom& g,
                                           float (*dst)[DP + 1], float mul) {
    for (int e = threadIdx.x; e < g.NP * DP; e += 256) {
        const int t = e / DP, d = e - t * DP;
        float v = 0.f;
        if (t < g.N && d < g.hd) v = src[rows[t] * ld + col0 + d] * mul;
        dst[t][d] = v;
    }
}

template <int DP>
__global__ __launch_bounds__(256) void swin_wattn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                             float* __restrict__ lse, WinGeom g, float scale) {
    __shared__ float Qs[WT][DP + 1], Ks[WT][DP + 1], Vs[WT][DP + 1];
    __shared__ float Ss[WT][SP];
    __shared__ int64_t rows[WT];
    const int win = blockIdx.x, h = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C3 = 3 * g.C;
    if (threadIdx.x < g.N) rows[threadIdx.x] = win_token_row(g, win, threadIdx.x);
    __syncthreads();
    load_slice<DP>(qkv, C3, h * g.hd, rows, g, Qs, scale);
    load_slice<DP>(qkv, C3, g.C + h * g.hd, rows, g, Ks, 1.f);
    load_slice<DP>(qkv, C3, 2 * g.C + h * g.hd, rows, g, Vs, 1.f);
    __syncthreads();
    const int nt = g.NP / 32;
    const int kd = (g.hd + 1) & ~1;
    if (wave < nt * nt) {   // S tile (ti, tj)
        const int ti = wave / nt, tj = wave - ti * nt;
        const floatx16 acc = mfma_tile(&Qs[ti * 32][0], DP + 1, 1, &Ks[tj * 32][0], 1, DP + 1, kd, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) Ss[ti * 32 + acc_row(r, lane)][tj * 32 + (lane & 31)] = acc[r];
    }
    __syncthreads();
    // row softmax over the N keys (one wave per row)
    for (int i = wave; i < g.N; i += 4) {
        const float v = lane < g.N ? Ss[i][lane] : -INFINITY;
        const float mx = wave_max(v);
        const float e = lane < g.N ? expf(v - mx) : 0.f;
        const float sum = wave_sum(e);
        if (lane < g.NP) Ss[i][lane] = e / sum;
        if (lse && lane == 0) lse[rows[i] * g.heads + h] = mx + logf(sum);
    }
    __syncthreads();
    const int nd = DP / 32;
    if (wave < nt * nd) {   // O tile (ti, td) = P V
        const int ti = wave / nd, td = wave - ti * nd;
        const floatx16 acc = mfma_tile(&Ss[ti * 32][0], SP, 1, &Vs[0][td * 32], DP + 1, 1, (g.N + 1) & ~1, lane);
        const int d = td * 32 + (lane & 31);
        if (d < g.hd) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = ti * 32 + acc_row(r, lane);
                if (i < g.N) out[rows[i] * g.C + h * g.hd + d] = acc[r];
            }
        }
    }
}

template <int DP>
__global__ __launch_bounds__(256) void swin_wattn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                             const float* __restrict__ dout, const float* __restrict__ lse,
                                                             float* __restrict__ dqkv, WinGeom g, float scale) {
    __shared__ float Qs[WT][DP + 1], Ks[WT][DP + 1], Vs[WT][DP + 1], dOs[WT][DP + 1];
    __shared__ float Ps[WT][SP], dSs[WT][SP];
    __shared__ float Dv[WT], Ls[WT];
    __shared__ int64_t rows[WT];
    const int win = blockIdx.x, h = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C3 = 3 * g.C;
    if (threadIdx.x < g.N) rows[threadIdx.x] = win_token_row(g, win, threadIdx.x);
    __syncthreads();
    load_slice<DP>(qkv, C3, h * g.hd, rows, g, Qs, scale);
    load_slice<DP>(qkv, C3, g.C + h * g.hd, rows, g, Ks, 1.f);
    load_slice<DP>(qkv, C3, 2 * g.C + h * g.hd, rows, g, Vs, 1.f);
    load_slice<DP>(dout, g.C, h * g.hd, rows, g, dOs, 1.f);
    // D_i = sum_d dO[i][d] O[i][d] (one wave per row), lse_i
    for (int i = wave; i < g.NP; i += 4) {
        float d = 0.f;
        if (i < g.N && lane < g.hd) d = dout[rows[i] * g.C + h * g.hd + lane] * o[rows[i] * g.C + h * g.hd + lane];
        d = wave_sum(d);
        if (lane == 0) {
            Dv[i] = d;
            Ls[i] = i < g.N ? lse[rows[i] * g.heads + h] : 0.f;
        }
    }
    __syncthreads();
    const int nt = g.NP / 32, nd = DP / 32;
    const int kd = (g.hd + 1) & ~1, kn = (g.N + 1) & ~1;
    if (wave < nt * nt) {   // P and dS tile (ti, tj): same wave, same register layout
        const int ti = wave / nt, tj = wave - ti * nt;
        const floatx16 s = mfma_tile(&Qs[ti * 32][0], DP + 1, 1, &Ks[tj * 32][0], 1, DP + 1, kd, lane);
        const floatx16 dp = mfma_tile(&dOs[ti * 32][0], DP + 1, 1, &Vs[tj * 32][0], 1, DP + 1, kd, lane);
        const int j = tj * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = ti * 32 + acc_row(r, lane);
            const float p = (i < g.N && j < g.N) ? expf(s[r] - Ls[i]) : 0.f;
            Ps[i][j] = p;
            dSs[i][j] = p * (dp[r] - Dv[i]);
        }
    }
    __syncthreads();
    if (wave < nt * nd) {
        const int ti = wave / nd, td = wave - ti * nd;
        const int d = td * 32 + (lane & 31);
        // dQ = scale dS K,  dK = dS^T (scale Q),  dV = P^T dO   (row tile ti of the tokens, column tile td of the head)
        const floatx16 dq = mfma_tile(&dSs[ti * 32][0], SP, 1, &Ks[0][td * 32], DP + 1, 1, kn, lane);
        const floatx16 dk = mfma_tile(&dSs[0][ti * 32], 1, SP, &Qs[0][td * 32], DP + 1, 1, kn, lane);
        const floatx16 dv = mfma_tile(&Ps[0][ti * 32], 1, SP, &dOs[0][td * 32], DP + 1, 1, kn, lane);
        if (d < g.hd) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = ti * 32 + acc_row(r, lane);
                if (i < g.N) {
                    float* row = dqkv + rows[i] * C3 + h * g.hd + d;
                    row[0] = scale * dq[r];
                    row[g.C] = dk[r];
                    row[2 * g.C] = dv[r];
                }
            }
        }
    }
}

// erf GELU (torch.nn.GELU default) and its derivative
__global__ void gelu_fwd_kernel(const float* __restrict__ h, float* __restrict__ g, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float x = h[e];
        g[e] = 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
    }
}
__global__ void gelu_bwd_kernel(const float* __restrict__ h, float* __restrict__ dg, int64_t n) {   // in place: dh = dg gelu'(h)
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float x = h[e];
        const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
        const float pdf = 0.39894228040143268f * expf(-0.5f * x * x);
        dg[e] = dg[e] * (cdf + x * pdf);
    }
}

// dir 0: y = (x - mean[c]) * r;  dir 1: y = x / r + mean[c]   (NCHW; mean may be null)
__global__ void img_affine_kernel(const float* __restrict__ x, const float* __restrict__ mean, float* __restrict__ y, int C, int HW,
                                  int64_t n, float r, int dir) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float m = mean ? mean[(e / HW) % C] : 0.f;
        y[e] = dir == 0 ? (x[e] - m) * r : x[e] / r + m;
    }
}

int check_window(int B, int H, int W, int C, int heads, int window, int shift, const char* who) {
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "%s: B=%d H=%d W=%d C=%d (C must be a positive multiple of 4)", who, B,
                   H, W, C);
    DCPT_CHECK_ARG(heads > 0 && C % heads == 0 && C / heads <= 64, "%s: C=%d heads=%d (C %% heads == 0, head_dim <= 64)", who, C, heads);
    DCPT_CHECK_ARG(window > 0 && window * window <= WT, "%s: window size %d (ws^2 must be <= %d)", who, window, WT);
    DCPT_CHECK_ARG(H % window == 0 && W % window == 0, "%s: H=%d W=%d must be multiples of the window size %d", who, H, W, window);
    DCPT_CHECK_ARG(shift >= 0 && shift < window, "%s: shift %d must be in [0, window)", who, shift);
    return DCPT_OK;
}

int launch_wattn_fwd(const float* qkv, float* out, float* lse, const WinGeom& g, hipStream_t s) {
    const dim3 grid((unsigned)(g.B * g.nwy * g.nwx), (unsigned)g.heads);
    const float scale = 1.f / sqrtf((float)g.hd);
    trace_tag("swin_wattn_fwd");
    if (g.hd <= 32) swin_wattn_fwd_kernel<32><<<grid, dim3(256), 0, s>>>(qkv, out, lse, g, scale);
    else swin_wattn_fwd_kernel<64><<<grid, dim3(256), 0, s>>>(qkv, out, lse, g, scale);
    DCPT_CHECK_LAUNCH("swin_wattn_fwd");
    return DCPT_OK;
}

int launch_wattn_bwd(const float* qkv, const float* o, const float* dout, const float* lse, float* dqkv, const WinGeom& g, hipStream_t s) {
    const dim3 grid((unsigned)(g.B * g.nwy * g.nwx), (unsigned)g.heads);
    const float scale = 1.f / sqrtf((float)g.hd);
    trace_tag("swin_wattn_bwd");
    if (g.hd <= 32) swin_wattn_bwd_kernel<32><<<grid, dim3(256), 0, s>>>(qkv, o, dout, lse, dqkv, g, scale);
    else swin_wattn_bwd_kernel<64><<<grid, dim3(256), 0, s>>>(qkv, o, dout, lse, dqkv, g, scale);
    DCPT_CHECK_LAUNCH("swin_wattn_bwd");
    return DCPT_OK;
}

// ---- attention half workspace ----------------------------------------------------------------------
struct AttnWs {
    float *mu, *rstd, *qkv, *att;     // forward intermediates when the caller keeps nothing
    float *wT_proj, *wT_qkv;          // [C][C], [C][3C]
    float *datt, *dqkv, *dxn;         // [M][C], [M][3C], [M][C]
    float *slab, *colsum, *lnpart;
    int ln_nblk;
};

size_t attn_layout(int B, int H, int W, int C, int backward, void* base, size_t bytes, AttnWs* out) {
    WsAlloc a(base, bytes);
    AttnWs w{};
    const int64_t M = (int64_t)B * H * W;
    if (!backward) {
        w.mu = a.get<float>((size_t)M);
        w.rstd = a.get<float>((size_t)M);
        w.qkv = a.get<float>((size_t)M * 3 * C);
        w.att = a.get<float>((size_t)M * C);
    } else {
        w.wT_proj = a.get<float>((size_t)C * C);
        w.wT_qkv = a.get<float>((size_t)3 * C * C);
        w.datt = a.get<float>((size_t)M * C);
        w.dqkv = a.get<float>((size_t)M * 3 * C);
        w.dxn = a.get<float>((size_t)M * C);
        size_t sl = 0, cs = 0;
        wgrad_need(M, C, C, &sl, &cs);
        wgrad_need(M, 3 * C, C, &sl, &cs);
        w.slab = a.get<float>(sl);
        w.colsum = a.get<float>(cs);
        w.ln_nblk = ln_bwd_num_blocks(M, C);
        w.lnpart = a.get<float>((size_t)w.ln_nblk * 3 * C);
    }
    if (out) *out = w;
    return a.off;
}

// ---- MLP half workspace ----------------------------------------------------------------------------
struct MlpWs {
    float *mu, *rstd, *h;   // forward intermediates when the caller keeps nothing
    float *g;               // [M][hidden] gelu(h)
    float *wT2, *wT1;       // [hidden][C], [C][hidden]
    float *dh, *dxn;        // [M][hidden], [M][C]
    float *slab, *colsum, *lnpart;
    int ln_nblk;
};

size_t mlp_layout(int B, int H, int W, int C, int hidden, int backward, void* base, size_t bytes, MlpWs* out) {
    WsAlloc a(base, bytes);
    MlpWs w{};
    const int64_t M = (int64_t)B * H * W;
    w.g = a.get<float>((size_t)M * hidden);
    if (!backward) {
        w.mu = a.get<float>((size_t)M);
        w.rstd = a.get<float>((size_t)M);
        w.h = a.get<float>((size_t)M * hidden);
    } else {
        w.wT2 = a.get<float>((size_t)hidden * C);
        w.wT1 = a.get<float>((size_t)C * hidden);
        w.dh = a.get<float>((size_t)M * hidden);
        w.dxn = a.get<float>((size_t)M * C);
        size_t sl = 0, cs = 0;
        wgrad_need(M, C, hidden, &sl, &cs);
        wgrad_need(M, hidden, C, &sl, &cs);
        w.slab = a.get<float>(sl);
        w.colsum = a.get<float>(cs);
        w.ln_nblk = ln_bwd_num_blocks(M, C);
        w.lnpart = a.get<float>((size_t)w.ln_nblk * 3 * C);
    }
    if (out) *out = w;
    return a.off;
}

// ---- 3x3 conv with bias and residual workspace --------------------------------------------------------
struct ConvResWs {
    float *wp;              // packed weights [C][9C]
    float *slab, *colsum;
};

size_t convres_layout(int B, int H, int W, int C, int backward, void* base, size_t bytes, ConvResWs* out) {
    WsAlloc a(base, bytes);
    ConvResWs w{};
    const int64_t M = (int64_t)B * H * W;
    w.wp = a.get<float>((size_t)9 * C * C);
    if (backward) {
        size_t sl = 0, cs = 0;
        wgrad_need(M, C, 9 * C, &sl, &cs);
        w.slab = a.get<float>(sl);
        w.colsum = a.get<float>(cs);
    }
    if (out) *out = w;
    return a.off;
}

}  // namespace

// =====================================================================================================
extern "C" size_t dcpt_swin_attn_ws_bytes(int B, int H, int W, int C, int heads, int backward) {
    (void)heads;
    return attn_layout(B, H, W, C, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_swin_attn_fwd(const dcpt_swin_attn_params* p, const float* x, float* y, const dcpt_swin_attn_saved* sv, void* ws,
                                  size_t ws_bytes, int B, int H, int W, int C, int heads, int window, int shift, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && x && y && p->norm_w && p->norm_b && p->qkv_w && p->qkv_b && p->proj_w && p->proj_b, "swin_attn_fwd: null argument");
    DCPT_CHECK_ARG(!sv || (sv->mu && sv->rstd && sv->qkv && sv->att && sv->lse), "swin_attn_fwd: null field in saved (pass saved = NULL to keep nothing)");
    DCPT_TRY(check_window(B, H, W, C, heads, window, shift, "swin_attn_fwd"));
    AttnWs w;
    const size_t need = attn_layout(B, H, W, C, 0, ws, ws_bytes, &w);
    DCPT_CHECK_WS("swin_attn_fwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    float* mu = sv ? sv->mu : w.mu;
    float* rstd = sv ? sv->rstd : w.rstd;
    float* qkv = sv ? sv->qkv : w.qkv;
    float* att = sv ? sv->att : w.att;
    DCPT_TRY(launch_ln_stats(x, mu, rstd, M, C, SWIN_LN_EPS, s));
    GemmNT g = gemm_nt_linear(x, C, M, C, p->qkv_w, 3 * C, qkv, 3 * C);
    g.bias = p->qkv_b; g.mu = mu; g.rstd = rstd; g.lnw = p->norm_w; g.lnb = p->norm_b;
    DCPT_TRY(launch_gemm_nt(g, A_LN, E_BIAS, s));
    DCPT_TRY(launch_wattn_fwd(qkv, att, sv ? sv->lse : nullptr, win_geom(B, H, W, C, heads, window, shift), s));
    g = gemm_nt_linear(att, C, M, C, p->proj_w, C, y, C);
    g.res = x; g.bias = p->proj_b;
    return launch_gemm_nt(g, A_PLAIN, E_RESID, s);
}

extern "C" int dcpt_swin_attn_bwd(const dcpt_swin_attn_params* p, const dcpt_swin_attn_params_grads* gr, const float* x,
                                  const dcpt_swin_attn_saved* sv, const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W,
                                  int C, int heads, int window, int shift, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && gr && x && sv && dy && dx && p->norm_w && p->norm_b && p->qkv_w && p->qkv_b && p->proj_w && p->proj_b,
                   "swin_attn_bwd: null argument");
    DCPT_CHECK_ARG(sv->mu && sv->rstd && sv->qkv && sv->att && sv->lse, "swin_attn_bwd: null field in saved");
    DCPT_CHECK_ARG(gr->norm_w && gr->norm_b && gr->qkv_w && gr->qkv_b && gr->proj_w && gr->proj_b, "swin_attn_bwd: null gradient");
    DCPT_TRY(check_window(B, H, W, C, heads, window, shift, "swin_attn_bwd"));
    AttnWs w;
    const size_t need = attn_layout(B, H, W, C, 1, ws, ws_bytes, &w);
    DCPT_CHECK_WS("swin_attn_bwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    // proj: d(att) = dy Wproj;  dWproj = dy^T att, dbproj = colsum(dy)
    DCPT_TRY(launch_wpack(p->proj_w, w.wT_proj, nullptr, C, C, WP_TRANSPOSE, s));
    DCPT_TRY(launch_gemm_nt(gemm_nt_linear(dy, C, M, C, w.wT_proj, C, w.datt, C), A_PLAIN, E_PLAIN, s));
    GemmTN tp{};
    DCPT_TRY(launch_wgrad(tp, A_PLAIN, dy, C, C, sv->att, C, C, M, w.slab, w.colsum, gr->proj_w, gr->proj_b, WR_PLAIN, s));
    // windowed attention
    DCPT_TRY(launch_wattn_bwd(sv->qkv, sv->att, w.datt, sv->lse, w.dqkv, win_geom(B, H, W, C, heads, window, shift), s));
    // qkv: d(LN1 x) = dqkv Wqkv;  dWqkv = dqkv^T LN1(x) (LayerNorm in the operand loader), dbqkv = colsum(dqkv)
    DCPT_TRY(launch_wpack(p->qkv_w, w.wT_qkv, nullptr, 3 * C, C, WP_TRANSPOSE, s));
    DCPT_TRY(launch_gemm_nt(gemm_nt_linear(w.dqkv, 3 * C, M, 3 * C, w.wT_qkv, C, w.dxn, C), A_PLAIN, E_PLAIN, s));
    tp.mu = sv->mu; tp.rstd = sv->rstd; tp.lnw = p->norm_w; tp.lnb = p->norm_b;
    DCPT_TRY(launch_wgrad(tp, A_LN, w.dqkv, 3 * C, 3 * C, x, C, C, M, w.slab, w.colsum, gr->qkv_w, gr->qkv_b, WR_PLAIN, s));
    // dx = dy + LN-backward
    DCPT_TRY(launch_ln_bwd(w.dxn, x, sv->mu, sv->rstd, p->norm_w, dy, dx, w.lnpart, w.ln_nblk, M, C, s));
    return launch_colpart_reduce(w.lnpart, w.ln_nblk, 3, C, gr->norm_w, gr->norm_b, nullptr, s);
}

// =====================================================================================================
extern "C" size_t dcpt_swin_mlp_ws_bytes(int B, int H, int W, int C, int hidden, int backward) {
    return mlp_layout(B, H, W, C, hidden, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_swin_mlp_fwd(const dcpt_swin_mlp_params* p, const float* x, float* y, const dcpt_swin_mlp_saved* sv, void* ws,
                                 size_t ws_bytes, int B, int H, int W, int C, int hidden, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && x && y && p->norm_w && p->norm_b && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, "swin_mlp_fwd: null argument");
    DCPT_CHECK_ARG(!sv || (sv->mu && sv->rstd && sv->h), "swin_mlp_fwd: null field in saved (pass saved = NULL to keep nothing)");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && hidden > 0 && hidden % 4 == 0,
                   "swin_mlp_fwd: C=%d hidden=%d (multiples of 4)", C, hidden);
    MlpWs w;
    const size_t need = mlp_layout(B, H, W, C, hidden, 0, ws, ws_bytes, &w);
    DCPT_CHECK_WS("swin_mlp_fwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    float* mu = sv ? sv->mu : w.mu;
    float* rstd = sv ? sv->rstd : w.rstd;
    float* h = sv ? sv->h : w.h;
    DCPT_TRY(launch_ln_stats(x, mu, rstd, M, C, SWIN_LN_EPS, s));
    GemmNT g = gemm_nt_linear(x, C, M, C, p->fc1_w, hidden, h, hidden);
    g.bias = p->fc1_b; g.mu = mu; g.rstd = rstd; g.lnw = p->norm_w; g.lnb = p->norm_b;
    DCPT_TRY(launch_gemm_nt(g, A_LN, E_BIAS, s));
    gelu_fwd_kernel<<<dim3(ew_grid(M * hidden)), dim3(256), 0, s>>>(h, w.g, M * hidden);
    DCPT_CHECK_LAUNCH("swin_gelu_fwd");
    g = gemm_nt_linear(w.g, hidden, M, hidden, p->fc2_w, C, y, C);
    g.res = x; g.bias = p->fc2_b;
    return launch_gemm_nt(g, A_PLAIN, E_RESID, s);
}

extern "C" int dcpt_swin_mlp_bwd(const dcpt_swin_mlp_params* p, const dcpt_swin_mlp_params_grads* gr, const float* x,
                                 const dcpt_swin_mlp_saved* sv, const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W,
                                 int C, int hidden, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && gr && x && sv && dy && dx && p->norm_w && p->norm_b && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b,
                   "swin_mlp_bwd: null argument");
    DCPT_CHECK_ARG(sv->mu && sv->rstd && sv->h, "swin_mlp_bwd: null field in saved");
    DCPT_CHECK_ARG(gr->norm_w && gr->norm_b && gr->fc1_w && gr->fc1_b && gr->fc2_w && gr->fc2_b, "swin_mlp_bwd: null gradient");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && hidden > 0 && hidden % 4 == 0,
                   "swin_mlp_bwd: C=%d hidden=%d (multiples of 4)", C, hidden);
    MlpWs w;
    const size_t need = mlp_layout(B, H, W, C, hidden, 1, ws, ws_bytes, &w);
    DCPT_CHECK_WS("swin_mlp_bwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    gelu_fwd_kernel<<<dim3(ew_grid(M * hidden)), dim3(256), 0, s>>>(sv->h, w.g, M * hidden);   // the fc2 operand, recomputed
    DCPT_CHECK_LAUNCH("swin_gelu_fwd");
    // fc2: dg = dy W2;  dW2 = dy^T gelu(h), db2 = colsum(dy)
    DCPT_TRY(launch_wpack(p->fc2_w, w.wT2, nullptr, C, hidden, WP_TRANSPOSE, s));
    DCPT_TRY(launch_gemm_nt(gemm_nt_linear(dy, C, M, C, w.wT2, hidden, w.dh, hidden), A_PLAIN, E_PLAIN, s));
    GemmTN tp{};
    DCPT_TRY(launch_wgrad(tp, A_PLAIN, dy, C, C, w.g, hidden, hidden, M, w.slab, w.colsum, gr->fc2_w, gr->fc2_b, WR_PLAIN, s));
    gelu_bwd_kernel<<<dim3(ew_grid(M * hidden)), dim3(256), 0, s>>>(sv->h, w.dh, M * hidden);
    DCPT_CHECK_LAUNCH("swin_gelu_bwd");
    // fc1: d(LN2 x) = dh W1;  dW1 = dh^T LN2(x), db1 = colsum(dh)
    DCPT_TRY(launch_wpack(p->fc1_w, w.wT1, nullptr, hidden, C, WP_TRANSPOSE, s));
    DCPT_TRY(launch_gemm_nt(gemm_nt_linear(w.dh, hidden, M, hidden, w.wT1, C, w.dxn, C), A_PLAIN, E_PLAIN, s));
    tp.mu = sv->mu; tp.rstd = sv->rstd; tp.lnw = p->norm_w; tp.lnb = p->norm_b;
    DCPT_TRY(launch_wgrad(tp, A_LN, w.dh, hidden, hidden, x, C, C, M, w.slab, w.colsum, gr->fc1_w, gr->fc1_b, WR_PLAIN, s));
    DCPT_TRY(launch_ln_bwd(w.dxn, x, sv->mu, sv->rstd, p->norm_w, dy, dx, w.lnpart, w.ln_nblk, M, C, s));
    return launch_colpart_reduce(w.lnpart, w.ln_nblk, 3, C, gr->norm_w, gr->norm_b, nullptr, s);
}

// =====================================================================================================
extern "C" size_t dcpt_conv3x3_res_ws_bytes(int B, int H, int W, int C, int backward) {
    return convres_layout(B, H, W, C, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_conv3x3_res_fwd(const float* x, const float* w, const float* bias, const float* res, float* y, void* ws, size_t ws_bytes,
                                    int B, int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(x && w && bias && res && y, "conv3x3_res_fwd: null argument");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "conv3x3_res_fwd: C=%d must be a positive multiple of 4", C);
    ConvResWs cw;
    const size_t need = convres_layout(B, H, W, C, 0, ws, ws_bytes, &cw);
    DCPT_CHECK_WS("conv3x3_res_fwd", ws, ws_bytes, need);
    trace_tag("swin_conv3x3_res_fwd");
    DCPT_TRY(launch_wpack(w, cw.wp, nullptr, C, 9 * C, WP_CONV3, s));
    GemmNT g = gemm_nt_conv3(x, B, H, W, C, cw.wp, C, y, C);
    g.bias = bias; g.res = res;
    return launch_gemm_nt(g, A_CONV3, E_RESID, s);
}

extern "C" int dcpt_conv3x3_res_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, void* ws,
                                    size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(dy && x && w && dx && dw && dbias, "conv3x3_res_bwd: null argument");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "conv3x3_res_bwd: C=%d must be a positive multiple of 4", C);
    ConvResWs cw;
    const size_t need = convres_layout(B, H, W, C, 1, ws, ws_bytes, &cw);
    DCPT_CHECK_WS("conv3x3_res_bwd", ws, ws_bytes, need);
    trace_tag("swin_conv3x3_res_bwd");
    return launch_conv3_bwd(dy, x, w, cw.wp, B, H, W, C, C, E_PLAIN, nullptr, 0.f, dx, cw.slab, cw.colsum, dw, dbias, s);
}

// =====================================================================================================
extern "C" int dcpt_img_affine(const float* x, const float* mean, float* y, int B, int C, int HW, float r, int dir, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && y && B > 0 && C > 0 && HW > 0 && (dir == 0 || dir == 1) && r != 0.f, "img_affine: bad argument");
    const int64_t n = (int64_t)B * C * HW;
    img_affine_kernel<<<dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream>>>(x, mean, y, C, HW, n, r, dir);
    DCPT_CHECK_LAUNCH("img_affine");
    return DCPT_OK;
}
