// SwinIR inference on bf16 activation storage (reference basicsr/archs/swinir_arch.py, the DCPT variant: no relative-position bias, no shift
// mask; the fp32 twins are in swin.hip):
//   attention half  y = bf16(x + proj(WMSA_shift(qkv(LN1(x)))))   dcpt_swin_attn_fwd_bf16
//   MLP half        y = bf16(x + fc2(gelu(fc1(LN2(x)))))          dcpt_swin_mlp_fwd_bf16
//   LayerNorm       y = bf16(LN(x) * w + b)                       dcpt_ln_pad_fwd_bf16   (patch_embed.norm, the final norm)
// Forward only: nothing is kept for a backward pass, there is none.  The RSTB conv, conv_after_body, conv_first and conv_last are the existing
// dcpt_conv3x3_res_fwd_bf16 / dcpt_conv3x3_in_fwd_bf16 / dcpt_conv3x3_out_fwd_bf16 at the padded width.
//
// FP32 RESIDUAL STREAM (the *_bf16_res32 entry points, act_dtype "bf16_res32"): the map x that runs through the residual adds is fp32 padded
// rows [M][Cp]; everything else is as above.  The LayerNorm reads the fp32 rows (same statistics, same bf16 output), the proj / fc2 GEMMs end
// in EB_RESID32 (acc + bias + x in fp32, stored as fp32 rows, optionally also as the bf16 image an RSTB conv reads): the stream is never
// rounded, every GEMM operand is still bf16.  One host path serves both forms (attn_run / mlp_run below).
//
// PADDED ROWS.  SwinIR's default width is 180 with 6 heads of 30 channels; every bf16 kernel of the library works on 16-byte rows.  The rule:
//   Cp  = C rounded up to a multiple of 8 (184 for 180, 40 for 36): token maps are bf16 NHWC rows [M][Cp], M = B*H*W
//   hdp = hd rounded up to a multiple of 8 (32 for 30, 8 for 6):    qkv is [M][3*heads*hdp], slice (s, h, d) at column (s*heads + h)*hdp + d,
//                                                                   the attention output is [M][heads*hdp]
// and ONE invariant makes the padding free: pad columns hold exact zeros everywhere.  The zeros come from the operands the caller builds once
// per parameter version -- weight operand images with zero rows for pad outputs and zero columns for pad inputs, zero-padded biases and
// LayerNorm vectors -- so a GEMM writes 0 into pad columns, the residual epilogue adds 0 to 0, padded head channels add 0 to q.k and give 0
// in P.V, and the existing GEMM / conv3 / edge kernels serve unchanged at the padded width.  The proj image [Cp][heads*hdp] carries the
// column map from padded heads back to channels.  Only the LayerNorm has to know C: its statistics run over the C real channels and it writes
// the pad columns as 0 itself.
//
// Storage points (where a value is rounded to bf16): the weight operand images, LN output, qkv, P, the attention output, proj + residual,
// fc1 + GELU, fc2 + residual.  Biases, LayerNorm statistics, scores, softmax and every accumulation are fp32.
//
// WINDOW KERNEL (swin_wattn_bf16_kernel).  Roll and window partition are addressing (swin_win.h, the fp32 kernel's map).  One WAVE per
// (window, head) pair, four consecutive pairs per 256-thread workgroup -- neighbouring heads of one window, whose qkv columns are
// neighbours in memory; a wave never talks to another one.  Per pair, with NP = 32 or 64 token slots and DP = 32 or 64 head-channel slots:
//   S^T = K Q^T  on v_mfma_f32_32x32x16_bf16: both operands are 16-byte GLOBAL loads straight into MFMA operand registers (lane = token,
//         8 consecutive head channels), no LDS.  The transposed product leaves lane (i, half) holding query i's scores against keys
//         j = 32 tj + (r & 3) + 8 (r >> 2) + 4 half: the scale hd^-0.5 (the REAL head dim) is applied to these fp32 values, keys j >= N are
//         masked, the row softmax is an in-lane reduction plus one exchange with lane ^ 32, all fp32 with max subtraction.
//   O^T = V^T P^T: the probabilities, rounded to bf16, ARE the B operand as they sit in the lane (the contraction index may be enumerated in
//         any order as long as both operands agree), so P never goes through LDS either.  Only V does: it is transposed on the way in
//         (Vt[d][j]) and read back as two 8-byte pieces per operand in the same key order.
//   O is accumulated in fp32, rounded once and written as 8-byte pieces (4 head channels of one token); padded head channels get the zeros
//   the zero V columns produce.  No lse, no atomics: every token of the map is written by exactly one wave.
// LDS: Vt only, 4 waves x DP x (NP + 4) bf16 = 17 408 bytes at the default geometry (NP 64, DP 32), 34 816 at DP 64, 9 216 at NP 32 / DP 32: four
// or more workgroups per CU by LDS; the 64 fp32 score registers per lane bound the occupancy before LDS does.  At ws = 8, hdp = 32 a pair is
// 16 MFMAs against 24 KB of scattered 64-byte reads: the kernel is bound by its loads, which is why Q and K skip LDS.
// Limits: ws^2 <= 64, hd <= hdp <= 64.
#include "bf16_ops.h"
#include "prof.h"
#include "swin_win.h"
#include "../../include/dcpt_hip.h"

namespace {

constexpr float SWIN_LN_EPS = 1e-5f;   // nn.LayerNorm default
constexpr int LNP_MAX_CP = 256;        // a row lives in 32 lanes of 8 channels

// ---- LayerNorm on padded rows ---------------------------------------------------------------------------------------------------------------
// y[m][c] = bf16((x[m][c] - mean) * rstd * w[c] + b[c]) for c < C, 0 for C <= c < Cp; statistics two-pass in fp32 over the C real channels
// (biased variance, eps inside the sqrt).  A row lives in 32 lanes (lane q: channels 8q .. 8q + 7), 8 rows per 256-thread block and pass.
// TIn: bf16_t (bf16 rows) or float (the fp32 residual stream: two 16-byte loads per lane, the values enter the statistics unrounded).
template <typename TIn>
__global__ __launch_bounds__(256) void ln_pad_fwd_bf16_kernel(const TIn* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                              bf16_t* __restrict__ y, int64_t M, int C, int Cp, float eps) {
    const int q = threadIdx.x & 31, c0 = 8 * q;
    const bool cok = c0 < Cp;
    float ww[8], bb[8];
    bool real[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        real[e] = c0 + e < C;
        ww[e] = real[e] ? w[c0 + e] : 0.f;
        bb[e] = real[e] ? b[c0 + e] : 0.f;
    }
    const float invC = 1.0f / (float)C;
    for (int64_t rb = blockIdx.x; rb * 8 < M; rb += gridDim.x) {
        const int64_t row = rb * 8 + (threadIdx.x >> 5);
        const bool ok = row < M && cok;
        float v[8];
        if constexpr (sizeof(TIn) == 4) {
            float4 lo = f4_zero(), hi = f4_zero();
            if (ok) {
                const float* xr = x + row * (int64_t)Cp + c0;
                lo = *reinterpret_cast<const float4*>(xr);
                hi = *reinterpret_cast<const float4*>(xr + 4);
            }
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
            v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        } else {
            uint4 u = make_uint4(0u, 0u, 0u, 0u);
            if (ok) u = *reinterpret_cast<const uint4*>(x + row * (int64_t)Cp + c0);
            v[0] = bf_lo(u.x); v[1] = bf_hi(u.x); v[2] = bf_lo(u.y); v[3] = bf_hi(u.y);
            v[4] = bf_lo(u.z); v[5] = bf_hi(u.z); v[6] = bf_lo(u.w); v[7] = bf_hi(u.w);
        }
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += real[e] ? v[e] : 0.f;
        const float mean = group_sum(sum, 32) * invC;
        float sq = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] = real[e] ? v[e] - mean : 0.f;
            sq += v[e] * v[e];
        }
        const float rs = 1.0f / sqrtf(group_sum(sq, 32) * invC + eps);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = real[e] ? fmaf(v[e] * rs, ww[e], bb[e]) : 0.f;
        if (ok) {
            uint4 u;
            u.x = bf_pack(o[0], o[1]); u.y = bf_pack(o[2], o[3]); u.z = bf_pack(o[4], o[5]); u.w = bf_pack(o[6], o[7]);
            *reinterpret_cast<uint4*>(y + row * (int64_t)Cp + c0) = u;
        }
    }
}

bool ln_pad_ok(int64_t M, int C, int Cp) { return M > 0 && C > 0 && C <= Cp && Cp % 8 == 0 && Cp <= LNP_MAX_CP; }

// the map a half reads and adds to: bf16 rows (x32 == null) or the fp32 residual stream (x == null)
struct RowsIn {
    const bf16_t* x;
    const float* x32;
};

int launch_ln_pad_fwd_bf16(RowsIn in, const float* w, const float* b, bf16_t* y, int64_t M, int C, int Cp, float eps, hipStream_t s) {
    DCPT_CHECK_ARG(ln_pad_ok(M, C, Cp), "ln_pad_fwd_bf16: M=%lld C=%d Cp=%d (0 < C <= Cp, Cp a multiple of 8, at most %d)", (long long)M, C, Cp, LNP_MAX_CP);
    trace_tag(in.x32 ? "swin_bf16.ln_pad_fwd_f32in" : "swin_bf16.ln_pad_fwd");
    int64_t nb = cdiv64(M, 8);
    if (nb > 4096) nb = 4096;
    if (in.x32) ln_pad_fwd_bf16_kernel<float><<<dim3((unsigned)nb), dim3(256), 0, s>>>(in.x32, w, b, y, M, C, Cp, eps);
    else ln_pad_fwd_bf16_kernel<bf16_t><<<dim3((unsigned)nb), dim3(256), 0, s>>>(in.x, w, b, y, M, C, Cp, eps);
    DCPT_CHECK_LAUNCH("ln_pad_fwd_bf16");
    return DCPT_OK;
}

// the GEMM that closes a half: y = x + (A Bw^T + bias) -- bf16 rows (EB_RESID), or the fp32 stream with its optional bf16 image (EB_RESID32)
int launch_resid_gemm(GemmNTB g, RowsIn in, bf16_t* y, float* y32, hipStream_t s) {
    g.C = y;
    if (!in.x32) {
        g.res = in.x;
        return launch_gemm_nt_bf16(g, EB_RESID, s);
    }
    g.res32 = in.x32; g.C32 = y32;
    return launch_gemm_nt_bf16(g, EB_RESID32, s);
}

// ---- window attention -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bf16x8 ldg_bf8(const bf16_t* p, bool ok) {
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (ok) u = *reinterpret_cast<const uint4*>(p);
    return __builtin_bit_cast(bf16x8, u);
}

// NT: 32-token tiles per window (NP = 32 NT slots >= N = ws^2);  DP: head-channel slots (>= hdp)
template <int NT, int DP>
__global__ __launch_bounds__(256) void swin_wattn_bf16_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, WinGeom g, int hdp,
                                                              int64_t npairs, float scale) {
    constexpr int NP = 32 * NT, KS = DP / 16, TD = DP / 32, CH = DP / 8;
    constexpr int VS = NP + 4;   // Vt row stride in elements: 8-byte aligned rows, 2-dword skew between consecutive d
    __shared__ __attribute__((aligned(16))) bf16_t Vt[4][DP][VS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t pair = (int64_t)blockIdx.x * 4 + wave;
    const bool active = pair < npairs;
    const int win = active ? (int)(pair / g.heads) : 0;
    const int h = active ? (int)(pair - (int64_t)win * g.heads) : 0;
    const int HD = g.heads * hdp, ld = 3 * HD;
    const int N = g.N;

    // V -> Vt[d][j] (zeros for token slots >= N and channel slots >= hdp: a zero P meets no NaN, a pad channel gives an exact 0)
    for (int idx = lane; idx < NP * CH; idx += 64) {
        const int t = idx / CH, c = idx - t * CH;
        const bool ok = active && t < N && 8 * c < hdp;
        const int64_t row = ok ? win_token_row(g, win, t) : 0;
        const uint4 u = __builtin_bit_cast(uint4, ldg_bf8(qkv + row * ld + 2 * HD + h * hdp + 8 * c, ok));
        bf16_t* dst = &Vt[wave][8 * c][t];
        dst[0 * VS] = (bf16_t)(u.x & 0xffffu); dst[1 * VS] = (bf16_t)(u.x >> 16);
        dst[2 * VS] = (bf16_t)(u.y & 0xffffu); dst[3 * VS] = (bf16_t)(u.y >> 16);
        dst[4 * VS] = (bf16_t)(u.z & 0xffffu); dst[5 * VS] = (bf16_t)(u.z >> 16);
        dst[6 * VS] = (bf16_t)(u.w & 0xffffu); dst[7 * VS] = (bf16_t)(u.w >> 16);
    }

    // this lane's tokens as an operand row: t = 32 tile + li
    int64_t trow[NT];
    bool tok[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        const int t = 32 * ti + li;
        tok[ti] = active && t < N;
        trow[ti] = tok[ti] ? win_token_row(g, win, t) : 0;
    }

    // S^T tiles: acc[tj][ti][r] = score of query 32 ti + li against key 32 tj + (r & 3) + 8 (r >> 2) + 4 lh
    floatx16 acc[NT][NT];
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tj][ti][r] = 0.f;
    {
        bf16x8 kf[NT][KS], qf[NT][KS];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int d0 = 16 * ks + 8 * lh;
                const bool ok = tok[t] && d0 < hdp;
                const bf16_t* base = qkv + trow[t] * ld + h * hdp + d0;
                qf[t][ks] = ldg_bf8(base, ok);
                kf[t][ks] = ldg_bf8(base + HD, ok);
            }
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc[tj][ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[tj][ks], qf[ti][ks], acc[tj][ti], 0, 0, 0);
    }

    // row softmax in fp32 over the N valid keys; the probabilities, rounded to bf16, in MFMA operand order
    bf16x8 pf[NT][NT][2];   // [ti][tj][k-step]
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        float mx = -INFINITY;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * tj + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float sv = j < N ? acc[tj][ti][r] * scale : -INFINITY;
                acc[tj][ti][r] = sv;
                mx = fmaxf(mx, sv);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * tj + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float e = j < N ? expf(acc[tj][ti][r] - mx) : 0.f;
                acc[tj][ti][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                u32x4 w;
                w.x = bf_pack(acc[tj][ti][8 * s2 + 0] * inv, acc[tj][ti][8 * s2 + 1] * inv);
                w.y = bf_pack(acc[tj][ti][8 * s2 + 2] * inv, acc[tj][ti][8 * s2 + 3] * inv);
                w.z = bf_pack(acc[tj][ti][8 * s2 + 4] * inv, acc[tj][ti][8 * s2 + 5] * inv);
                w.w = bf_pack(acc[tj][ti][8 * s2 + 6] * inv, acc[tj][ti][8 * s2 + 7] * inv);
                pf[ti][tj][s2] = __builtin_bit_cast(bf16x8, w);
            }
    }
    __syncthreads();   // Vt is complete (each wave reads only its own slice; the barrier is uniform: no branch above leaves the kernel)

    // O^T = V^T P^T: rows d = 32 td + (r & 3) + 8 (r >> 2) + 4 lh, column = query 32 ti + li
#pragma unroll
    for (int td = 0; td < TD; ++td) {
        floatx16 oacc[NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[ti][r] = 0.f;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                // element e of the operand is key 32 tj + 16 s2 + 4 lh + (e & 3) + 8 (e >> 2): P's order above
                const bf16_t* vr = &Vt[wave][32 * td + li][32 * tj + 16 * s2 + 4 * lh];
                const u32x2 lo = *reinterpret_cast<const u32x2*>(vr), hi = *reinterpret_cast<const u32x2*>(vr + 8);
                u32x4 w;
                w.x = lo.x; w.y = lo.y; w.z = hi.x; w.w = hi.y;
                const bf16x8 vf = __builtin_bit_cast(bf16x8, w);
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) oacc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[ti][tj][s2], oacc[ti], 0, 0, 0);
            }
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            if (!tok[ti]) continue;
            bf16_t* orow = out + trow[ti] * HD + h * hdp;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * td + 8 * g4 + 4 * lh;
                if (d0 < hdp) {
                    u32x2 w;
                    w.x = bf_pack(oacc[ti][4 * g4 + 0], oacc[ti][4 * g4 + 1]);
                    w.y = bf_pack(oacc[ti][4 * g4 + 2], oacc[ti][4 * g4 + 3]);
                    *reinterpret_cast<u32x2*>(orow + d0) = w;
                }
            }
        }
    }
}

int launch_wattn_bf16(const bf16_t* qkv, bf16_t* out, const WinGeom& g, int hdp, hipStream_t s) {
    const int64_t npairs = (int64_t)g.B * g.nwy * g.nwx * g.heads;
    const dim3 grid((unsigned)cdiv64(npairs, 4));
    const float scale = 1.f / sqrtf((float)g.hd);
    trace_tag("swin_bf16.wattn_fwd");
    if (g.NP == 32) {
        if (hdp <= 32) swin_wattn_bf16_kernel<1, 32><<<grid, dim3(256), 0, s>>>(qkv, out, g, hdp, npairs, scale);
        else swin_wattn_bf16_kernel<1, 64><<<grid, dim3(256), 0, s>>>(qkv, out, g, hdp, npairs, scale);
    } else {
        if (hdp <= 32) swin_wattn_bf16_kernel<2, 32><<<grid, dim3(256), 0, s>>>(qkv, out, g, hdp, npairs, scale);
        else swin_wattn_bf16_kernel<2, 64><<<grid, dim3(256), 0, s>>>(qkv, out, g, hdp, npairs, scale);
    }
    DCPT_CHECK_LAUNCH("swin_wattn_bf16");
    return DCPT_OK;
}

// ---- argument checks (before the first launch; the workspace queries answer 0 without a device) -----------------------------------------------
// the limits launch_gemm_nt_bf16 enforces for the widest launch of a half (N columns over M rows)
// (the fp32-residual epilogue's own bound, 128 fp32 rows of Cp columns inside the 32-bit window, is implied by Cp <= LNP_MAX_CP: 132 KB)
bool rows_ok(int B, int H, int W, int C, int Cp, int Nmax) {
    static_assert(4.0 * (128.0 * LNP_MAX_CP + LNP_MAX_CP) < (double)WIN_BYTES, "EB_RESID32 rows of a half inside the buffer window");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C > Cp || Cp % 8 != 0 || Cp > LNP_MAX_CP) return false;
    if ((int64_t)H * W >= (1 << 30) || (int64_t)B * H * W >= (1ll << 40)) return false;
    const int64_t M = (int64_t)B * H * W;
    return Nmax > 0 && Nmax % 8 == 0 && Nmax < (1 << 20) && cdiv64(M, 128) * cdiv(Nmax, 32) < (1ll << 31) && cdiv64(M, 8) < (1ll << 31);
}
bool attn_ok(int B, int H, int W, int C, int Cp, int heads, int hdp, int window) {
    if (heads <= 0 || C <= 0 || C % heads != 0) return false;
    const int hd = C / heads;
    if (hdp % 8 != 0 || hdp < hd || hdp > 64) return false;
    if (window <= 0 || window * window > WT || H % window != 0 || W % window != 0) return false;
    if (!rows_ok(B, H, W, C, Cp, 3 * heads * hdp)) return false;
    return (int64_t)B * (H / window) * (W / window) * heads < (1ll << 33);
}
bool mlp_ok(int B, int H, int W, int C, int Cp, int hidden) { return hidden > 0 && hidden % 8 == 0 && rows_ok(B, H, W, C, Cp, hidden > Cp ? hidden : Cp); }

struct AttnWsB {
    bf16_t *xn, *qkv, *att;   // [M][Cp], [M][3 heads hdp], [M][heads hdp]
};
size_t attn_layout_b(int64_t M, int Cp, int HD, void* base, size_t bytes, AttnWsB* out) {
    WsAlloc a(base, bytes);
    AttnWsB w{};
    w.xn = a.get<bf16_t>((size_t)M * Cp);
    w.qkv = a.get<bf16_t>((size_t)M * 3 * HD);
    w.att = a.get<bf16_t>((size_t)M * HD);
    if (out) *out = w;
    return a.off;
}
struct MlpWsB {
    bf16_t *xn, *g;   // [M][Cp], [M][hidden]
};
size_t mlp_layout_b(int64_t M, int Cp, int hidden, void* base, size_t bytes, MlpWsB* out) {
    WsAlloc a(base, bytes);
    MlpWsB w{};
    w.xn = a.get<bf16_t>((size_t)M * Cp);
    w.g = a.get<bf16_t>((size_t)M * hidden);
    if (out) *out = w;
    return a.off;
}

// ---- the two halves, both storage forms of the residual map (in / y / y32 as launch_resid_gemm's) ------------------------------------------
int attn_run(const char* who, const dcpt_swin_attn_bf16_params* p, RowsIn in, bf16_t* y, float* y32, void* ws, size_t ws_bytes, int B, int H, int W,
             int C, int Cp, int heads, int hdp, int window, int shift, hipStream_t s) {
    DCPT_CHECK_ARG(p && (in.x || in.x32) && (y || y32) && p->norm_w && p->norm_b && p->qkv_w && p->qkv_b && p->proj_w && p->proj_b, "%s: null argument",
                   who);
    DCPT_CHECK_ARG(attn_ok(B, H, W, C, Cp, heads, hdp, window),
                   "%s: B=%d H=%d W=%d C=%d Cp=%d heads=%d hdp=%d window=%d (0 < C <= Cp, Cp a multiple of 8 up to %d, C %% heads == 0, "
                   "head_dim <= hdp <= 64 with hdp a multiple of 8, window^2 <= %d, H and W multiples of the window)",
                   who, B, H, W, C, Cp, heads, hdp, window, LNP_MAX_CP, WT);
    DCPT_CHECK_ARG(shift >= 0 && shift < window, "%s: shift %d must be in [0, window)", who, shift);
    const int64_t M = (int64_t)B * H * W;
    const int HD = heads * hdp;
    AttnWsB w;
    const size_t need = attn_layout_b(M, Cp, HD, ws, ws_bytes, &w);
    DCPT_CHECK_WS(who, ws, ws_bytes, need);
    trace_tag(in.x32 ? "swin_bf16.attn_fwd_res32" : "swin_bf16.attn_fwd");
    DCPT_TRY(launch_ln_pad_fwd_bf16(in, p->norm_w, p->norm_b, w.xn, M, C, Cp, SWIN_LN_EPS, s));
    GemmNTB g = gemm_ntb_linear(w.xn, Cp, M, Cp, p->qkv_w, 3 * HD, w.qkv, 3 * HD);
    g.bias = p->qkv_b;
    DCPT_TRY(launch_gemm_nt_bf16(g, EB_BIAS, s));
    DCPT_TRY(launch_wattn_bf16(w.qkv, w.att, win_geom(B, H, W, C, heads, window, shift), hdp, s));
    g = gemm_ntb_linear(w.att, HD, M, HD, p->proj_w, Cp, nullptr, Cp);
    g.bias = p->proj_b;
    return launch_resid_gemm(g, in, y, y32, s);
}

int mlp_run(const char* who, const dcpt_swin_mlp_bf16_params* p, RowsIn in, bf16_t* y, float* y32, void* ws, size_t ws_bytes, int B, int H, int W,
            int C, int Cp, int hidden, hipStream_t s) {
    DCPT_CHECK_ARG(p && (in.x || in.x32) && (y || y32) && p->norm_w && p->norm_b && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, "%s: null argument",
                   who);
    DCPT_CHECK_ARG(mlp_ok(B, H, W, C, Cp, hidden),
                   "%s: B=%d H=%d W=%d C=%d Cp=%d hidden=%d (0 < C <= Cp, Cp a multiple of 8 up to %d, hidden a positive multiple of 8)", who, B, H, W, C,
                   Cp, hidden, LNP_MAX_CP);
    const int64_t M = (int64_t)B * H * W;
    MlpWsB w;
    const size_t need = mlp_layout_b(M, Cp, hidden, ws, ws_bytes, &w);
    DCPT_CHECK_WS(who, ws, ws_bytes, need);
    trace_tag(in.x32 ? "swin_bf16.mlp_fwd_res32" : "swin_bf16.mlp_fwd");
    DCPT_TRY(launch_ln_pad_fwd_bf16(in, p->norm_w, p->norm_b, w.xn, M, C, Cp, SWIN_LN_EPS, s));
    GemmNTB g = gemm_ntb_linear(w.xn, Cp, M, Cp, p->fc1_w, hidden, w.g, hidden);
    g.bias = p->fc1_b;
    DCPT_TRY(launch_gemm_nt_bf16(g, EB_BIASGELU, s));
    g = gemm_ntb_linear(w.g, hidden, M, hidden, p->fc2_w, Cp, nullptr, Cp);
    g.bias = p->fc2_b;
    return launch_resid_gemm(g, in, y, y32, s);
}

}  // namespace

// =====================================================================================================
extern "C" int dcpt_ln_pad_fwd_bf16(const uint16_t* x, const float* w, const float* b, uint16_t* y, int64_t M, int C, int Cp, float eps,
                                    dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && w && b && y, "ln_pad_fwd_bf16: null argument");
    return launch_ln_pad_fwd_bf16(RowsIn{x, nullptr}, w, b, y, M, C, Cp, eps, (hipStream_t)stream);
}

extern "C" int dcpt_ln_pad_fwd_bf16_res32(const float* x, const float* w, const float* b, uint16_t* y, int64_t M, int C, int Cp, float eps,
                                          dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && w && b && y, "ln_pad_fwd_bf16_res32: null argument");
    return launch_ln_pad_fwd_bf16(RowsIn{nullptr, x}, w, b, y, M, C, Cp, eps, (hipStream_t)stream);
}

// =====================================================================================================
extern "C" size_t dcpt_swin_attn_bf16_ws_bytes(int B, int H, int W, int C, int Cp, int heads, int hdp, int window) {
    if (!attn_ok(B, H, W, C, Cp, heads, hdp, window)) return 0;
    return attn_layout_b((int64_t)B * H * W, Cp, heads * hdp, nullptr, 0, nullptr);
}
// (the stream form keeps the same bf16 intermediates: LN output, qkv, attention output)
extern "C" size_t dcpt_swin_attn_bf16_res32_ws_bytes(int B, int H, int W, int C, int Cp, int heads, int hdp, int window) {
    return dcpt_swin_attn_bf16_ws_bytes(B, H, W, C, Cp, heads, hdp, window);
}

extern "C" int dcpt_swin_attn_fwd_bf16(const dcpt_swin_attn_bf16_params* p, const uint16_t* x, uint16_t* y, void* ws, size_t ws_bytes, int B, int H,
                                       int W, int C, int Cp, int heads, int hdp, int window, int shift, dcpt_stream_t stream) {
    return attn_run("swin_attn_fwd_bf16", p, RowsIn{x, nullptr}, y, nullptr, ws, ws_bytes, B, H, W, C, Cp, heads, hdp, window, shift, (hipStream_t)stream);
}

extern "C" int dcpt_swin_attn_fwd_bf16_res32(const dcpt_swin_attn_bf16_params* p, const float* x, float* y, void* ws, size_t ws_bytes, int B, int H,
                                             int W, int C, int Cp, int heads, int hdp, int window, int shift, dcpt_stream_t stream) {
    return attn_run("swin_attn_fwd_bf16_res32", p, RowsIn{nullptr, x}, nullptr, y, ws, ws_bytes, B, H, W, C, Cp, heads, hdp, window, shift,
                    (hipStream_t)stream);
}

// =====================================================================================================
extern "C" size_t dcpt_swin_mlp_bf16_ws_bytes(int B, int H, int W, int C, int Cp, int hidden) {
    if (!mlp_ok(B, H, W, C, Cp, hidden)) return 0;
    return mlp_layout_b((int64_t)B * H * W, Cp, hidden, nullptr, 0, nullptr);
}
extern "C" size_t dcpt_swin_mlp_bf16_res32_ws_bytes(int B, int H, int W, int C, int Cp, int hidden) {
    return dcpt_swin_mlp_bf16_ws_bytes(B, H, W, C, Cp, hidden);
}

extern "C" int dcpt_swin_mlp_fwd_bf16(const dcpt_swin_mlp_bf16_params* p, const uint16_t* x, uint16_t* y, void* ws, size_t ws_bytes, int B, int H,
                                      int W, int C, int Cp, int hidden, dcpt_stream_t stream) {
    return mlp_run("swin_mlp_fwd_bf16", p, RowsIn{x, nullptr}, y, nullptr, ws, ws_bytes, B, H, W, C, Cp, hidden, (hipStream_t)stream);
}

extern "C" int dcpt_swin_mlp_fwd_bf16_res32(const dcpt_swin_mlp_bf16_params* p, const float* x, float* y, uint16_t* y_bf16, void* ws, size_t ws_bytes,
                                            int B, int H, int W, int C, int Cp, int hidden, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(y, "swin_mlp_fwd_bf16_res32: null argument");
    return mlp_run("swin_mlp_fwd_bf16_res32", p, RowsIn{nullptr, x}, y_bf16, y, ws, ws_bytes, B, H, W, C, Cp, hidden, (hipStream_t)stream);
}
