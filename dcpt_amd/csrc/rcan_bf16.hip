// RCAN inference on bf16 activation storage (reference basicsr/archs/rcan_arch.py; the fp32 twins are in rcan.hip and swin.hip):
//   RCAB (:32-54, ChannelAttention :9-29)   y = bf16(x + res_scale * t * s)                        dcpt_rcab_fwd_bf16
//   group conv / conv_after_body (:79-82, :147)   y = bf16(res + conv3x3(x) + bias)                dcpt_conv3x3_res_fwd_bf16
//   Upsample stage (arch_util.py Upsample)   y = bf16(PixelShuffle(r)(conv3x3(x) + bias)), r 2 | 3   dcpt_conv3x3_ps_fwd_bf16
// Forward only: nothing is kept for a backward pass, there is none.
//
// FP32 RESIDUAL STREAM (the *_bf16_res32 entry points, act_dtype "bf16_res32"): the map S that runs through the residual adds is fp32 [M][C] with
// its bf16 image Sb = bf16(S) next to it; every conv reads Sb, h and t stay bf16, and
//   S' = S + res_scale * t * s              rcab_scale_res32_kernel: fp32 out and Sb' = bf16(S') in one pass
//   S' = S_in + conv(Sb) + bias             EB_RESID32 from the fp32 accumulator: fp32 out and / or its bf16 image (conv_after_body: bf16 only)
// The stream is never rounded.  One host path serves both forms (rcab_run / res_run below).
//
// Feature maps are bf16 NHWC rows [M][C] (M = B*H*W, C % 8 == 0); parameters are fp32.  Every conv is the implicit 3 x 3 form (conv3) of the
// bf16 NT GEMM (gemm_bf16.hip, fp32 accumulation) on the 128-row kernel, with the epilogues this file adds to it (gemm_bf16_epi.h):
//   h = bf16(relu(conv1(x) + b1))         EB_BIASRELU
//   t = bf16(conv2(h) + b2)               EB_BIASCOL: the per-image column sums are taken from the fp32 accumulator + bias BEFORE the rounding,
//                                         one partial row per (tile, image) pair in a fixed order -- no atomics, run-to-run bit-identical.
//                                         This GEMM tiles its rows per image, so the terms of an image's sum and their order do not depend on
//                                         the batch: a batched forward equals the one-image forwards bit for bit (tiled inference batches
//                                         tiles of equal shape, and a bf16 rounding downstream would amplify a last-bit difference of s)
//   s = sigmoid(W2 relu(W1 mean_hw(t) + b1') + b2')   rcan.hip's CA kernel on those fp32 sums (launch_rcan_ca_fwd): pooling, FCs, sigmoid fp32
//   y = bf16(x + res_scale * t * s)       rcab_scale_bf16_kernel below: 16-byte vectors, one rounding
// Storage points (where a value is rounded to bf16): the weight operand images, h, t, y, and the outputs of the other two entry points.
// Each conv's weight comes as its cached operand image (dcpt_conv_wpack_bf16_multi; the forward half is used) or is packed in the call.
// The pixel shuffle reads the cached image in the conv's own channel order: GEMM column (i r + j) C + c is conv channel c r^2 + i r + j, the
// GEMM's weight loader and bias load apply that map (EB_PSHUF), so no reordered copy of the weights exists and r = 3 takes the same path as
// r = 2 -- the GEMM's scatter epilogue writes the shuffled bf16 image directly, no intermediate map in any precision.
#include "bf16_ops.h"
#include "prof.h"
#include "../../include/dcpt_hip.h"

namespace {

__device__ __forceinline__ f8 bf8_ldg(const bf16_t* p) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    f8 o;
    o.lo = make_float4(bf_lo(w.x), bf_hi(w.x), bf_lo(w.y), bf_hi(w.y));
    o.hi = make_float4(bf_lo(w.z), bf_hi(w.z), bf_lo(w.w), bf_hi(w.w));
    return o;
}
__device__ __forceinline__ void bf8_stg(bf16_t* p, f8 v) {
    uint4 w;
    w.x = bf_pack(v.lo.x, v.lo.y);
    w.y = bf_pack(v.lo.z, v.lo.w);
    w.z = bf_pack(v.hi.x, v.hi.y);
    w.w = bf_pack(v.hi.z, v.hi.w);
    *reinterpret_cast<uint4*>(p) = w;
}

// y = bf16(x + rs * t * s[b][c])   (groups of 8 channels; C % 8 == 0; the expression of rcan.hip's rcab_scale_kernel)
__global__ __launch_bounds__(256) void rcab_scale_bf16_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ t, const float* __restrict__ s,
                                                              bf16_t* __restrict__ y, int64_t n8, int C, int64_t PC, float rs) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n8; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t el = 8 * e;
        const f8 sv = f8_ld(s + (el / PC) * C + el % C);
        const f8 xv = bf8_ldg(x + el), tv = bf8_ldg(t + el);
        f8 o;
        o.lo = make_float4(fmaf(rs * tv.lo.x, sv.lo.x, xv.lo.x), fmaf(rs * tv.lo.y, sv.lo.y, xv.lo.y), fmaf(rs * tv.lo.z, sv.lo.z, xv.lo.z),
                           fmaf(rs * tv.lo.w, sv.lo.w, xv.lo.w));
        o.hi = make_float4(fmaf(rs * tv.hi.x, sv.hi.x, xv.hi.x), fmaf(rs * tv.hi.y, sv.hi.y, xv.hi.y), fmaf(rs * tv.hi.z, sv.hi.z, xv.hi.z),
                           fmaf(rs * tv.hi.w, sv.hi.w, xv.hi.w));
        bf8_stg(y + el, o);
    }
}

// the stream form: S' = S + rs * t * s[b][c] stored in fp32 and Sb' = bf16(S'); x, y fp32, t and yb bf16 (the same expression)
__global__ __launch_bounds__(256) void rcab_scale_res32_kernel(const float* __restrict__ x, const bf16_t* __restrict__ t, const float* __restrict__ s,
                                                               float* __restrict__ y, bf16_t* __restrict__ yb, int64_t n8, int C, int64_t PC, float rs) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n8; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t el = 8 * e;
        const f8 sv = f8_ld(s + (el / PC) * C + el % C);
        const f8 xv = f8_ld(x + el), tv = bf8_ldg(t + el);
        f8 o;
        o.lo = make_float4(fmaf(rs * tv.lo.x, sv.lo.x, xv.lo.x), fmaf(rs * tv.lo.y, sv.lo.y, xv.lo.y), fmaf(rs * tv.lo.z, sv.lo.z, xv.lo.z),
                           fmaf(rs * tv.lo.w, sv.lo.w, xv.lo.w));
        o.hi = make_float4(fmaf(rs * tv.hi.x, sv.hi.x, xv.hi.x), fmaf(rs * tv.hi.y, sv.hi.y, xv.hi.y), fmaf(rs * tv.hi.z, sv.hi.z, xv.hi.z),
                           fmaf(rs * tv.hi.w, sv.hi.w, xv.hi.w));
        stg4(y + el, o.lo);
        stg4(y + el + 4, o.hi);
        bf8_stg(yb + el, o);
    }
}

// the limits launch_gemm_nt_bf16 enforces for a conv3 launch of Cout columns over a [B][H][W][C] map (checked here so that an entry point
// refuses before its first launch, and so that the workspace queries answer 0 without a device); channels <= 1024 as the cached operand images
bool conv3_ok(int B, int H, int W, int C, int Cout) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || C > 1024 || Cout <= 0 || Cout % 8 != 0) return false;
    if ((int64_t)H * W >= (1 << 30)) return false;
    const int64_t M = (int64_t)B * H * W;
    return (double)(130 + 2 * W + 2) * C * 2.0 < 1.0e9 && 9 * C < (1 << 20) && Cout < (1 << 20) && (double)Cout * 9.0 * C * 2.0 < 1.0e9 &&
           (cdiv64(M, 128) + B) * cdiv(Cout, 32) < (1ll << 31);   // (+ B: the conv2 GEMM of an RCAB tiles its rows per image)
}
bool rcab_ok(int B, int H, int W, int C, int Cr) { return conv3_ok(B, H, W, C, C) && Cr >= 1 && Cr <= C; }
bool ps_ok(int B, int H, int W, int C, int r) {
    return (r == 2 || r == 3) && conv3_ok(B, H, W, C, r * r * C) && (double)(130 + 2 * W) * (double)(r * r) * C * 2.0 < 1.0e9;
}

// the forward operand image [Cout][9 C] of a conv: the first half of its cached pack, or packed here into `wp`
int operand(const float* w, const void* pk, bf16_t* wp, int C, int Cout, const bf16_t** out, hipStream_t s) {
    if (pk) {
        *out = pk_fwd(pk);
        return DCPT_OK;
    }
    trace_tag("rcan_bf16.wpack_per_call");   // (not reached with the network's cached images)
    *out = wp;
    return launch_wpack_bf16_one(w, wp, Cout, 9 * C, 2, s);
}

struct RcabWsB {
    bf16_t *wp1, *wp2;   // operand images packed in the call (unused with cached ones)
    float* colpart;      // [(tiles_m + B - 1)][C] tile / image column sums of t
    bf16_t *h, *t;       // [M][C]
    float *pooled, *s;   // [B][C]
};
size_t rcab_layout(int B, int H, int W, int C, void* base, size_t bytes, RcabWsB* out) {
    WsAlloc a(base, bytes);
    RcabWsB w{};
    const int64_t M = (int64_t)B * H * W;
    w.wp1 = a.get<bf16_t>((size_t)9 * C * C);
    w.wp2 = a.get<bf16_t>((size_t)9 * C * C);
    w.colpart = a.get<float>((size_t)(cdiv64(M, 128) + B - 1) * C);
    w.h = a.get<bf16_t>((size_t)M * C);
    w.t = a.get<bf16_t>((size_t)M * C);
    w.pooled = a.get<float>((size_t)B * C);
    w.s = a.get<float>((size_t)B * C);
    if (out) *out = w;
    return a.off;
}

// ---- the RCAB and the residual conv, both storage forms of the residual map ---------------------------------------------------------------
// x: the bf16 map the convs read.  x32 == null: bf16 residual, y = bf16(x + ...).  x32 != null: the fp32 stream (x is its bf16 image), y32 = the
// new stream and y its bf16 image.
int rcab_run(const char* who, const dcpt_rcab_params* p, const void* wpacked1, size_t wpacked1_bytes, const void* wpacked2, size_t wpacked2_bytes,
             const bf16_t* x, const float* x32, bf16_t* y, float* y32, bool stream32, void* ws, size_t ws_bytes, int B, int H, int W, int C, int Cr,
             float res_scale, hipStream_t s) {
    DCPT_CHECK_ARG(p && x && y && (!stream32 || (x32 && y32)) && p->conv1_b && p->conv2_b && p->ca1_w && p->ca1_b && p->ca2_w && p->ca2_b,
                   "%s: null argument", who);
    DCPT_CHECK_ARG(rcab_ok(B, H, W, C, Cr), "%s: B=%d H=%d W=%d C=%d Cr=%d (C a positive multiple of 8 up to 1024, 1 <= Cr <= C, one map inside the 32-bit windows)",
                   who, B, H, W, C, Cr);
    DCPT_CHECK_ARG(p->conv1_w || wpacked1, "%s: null argument (weights)", who);
    DCPT_TRY(pk_check(wpacked1, wpacked1_bytes, C, C, 3, who));
    DCPT_CHECK_ARG(p->conv2_w || wpacked2, "%s: null argument (weights)", who);
    DCPT_TRY(pk_check(wpacked2, wpacked2_bytes, C, C, 3, who));
    RcabWsB w;
    const size_t need = rcab_layout(B, H, W, C, ws, ws_bytes, &w);
    DCPT_CHECK_WS(who, ws, ws_bytes, need);
    const int P = H * W;
    const int64_t M = (int64_t)B * P;
    trace_tag(stream32 ? "rcan_bf16.rcab_fwd_res32" : "rcan_bf16.rcab_fwd");
    const bf16_t *b1, *b2;
    DCPT_TRY(operand(p->conv1_w, wpacked1, w.wp1, C, C, &b1, s));
    DCPT_TRY(operand(p->conv2_w, wpacked2, w.wp2, C, C, &b2, s));
    // h = relu(conv1(x) + b1)
    GemmNTB g = gemm_ntb_conv3(x, B, H, W, C, b1, C, w.h, C);
    g.bias = p->conv1_b;
    DCPT_TRY(launch_gemm_nt_bf16(g, EB_BIASRELU, s));
    // t = conv2(h) + b2, and the per-image column sums of its fp32 values
    g = gemm_ntb_conv3(w.h, B, H, W, C, b2, C, w.t, C);
    g.bias = p->conv2_b; g.colpart = w.colpart; g.P = P;
    DCPT_TRY(launch_gemm_nt_bf16(g, EB_BIASCOL, s));
    DCPT_TRY(launch_rcan_ca_fwd(w.colpart, p->ca1_w, p->ca1_b, p->ca2_w, p->ca2_b, w.pooled, w.s, B, P, C, Cr, s));
    const int64_t n8 = M * C / 8;
    if (stream32) {
        trace_tag("rcan_bf16.scale_res32");
        rcab_scale_res32_kernel<<<dim3(ew_grid(n8)), dim3(256), 0, s>>>(x32, w.t, w.s, y32, y, n8, C, (int64_t)P * C, res_scale);
        DCPT_CHECK_LAUNCH("rcab_scale_res32");
    } else {
        rcab_scale_bf16_kernel<<<dim3(ew_grid(n8)), dim3(256), 0, s>>>(x, w.t, w.s, y, n8, C, (int64_t)P * C, res_scale);
        DCPT_CHECK_LAUNCH("rcab_scale_bf16");
    }
    return DCPT_OK;
}

// res: the bf16 residual (EB_RESID -> y), or res32: the fp32 one (EB_RESID32 -> y32 and / or y)
int res_run(const char* who, const bf16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, const float* bias, const bf16_t* res,
            const float* res32, bf16_t* y, float* y32, void* ws, size_t ws_bytes, int B, int H, int W, int C, hipStream_t s) {
    DCPT_CHECK_ARG(x && bias && (res || res32) && (y || y32), "%s: null argument", who);
    DCPT_CHECK_ARG(conv3_ok(B, H, W, C, C), "%s: B=%d H=%d W=%d C=%d (C a positive multiple of 8 up to 1024, one map inside the 32-bit windows)", who, B,
                   H, W, C);
    DCPT_CHECK_ARG(w || wpacked, "%s: null argument (weights)", who);
    DCPT_TRY(pk_check(wpacked, wpacked_bytes, C, C, 3, who));
    const size_t need = dcpt_conv3x3_res_bf16_ws_bytes(B, H, W, C);
    DCPT_CHECK_WS(who, ws, ws_bytes, need);
    trace_tag(res32 ? "rcan_bf16.res_fwd_res32" : "rcan_bf16.res_fwd");
    const bf16_t* bw;
    DCPT_TRY(operand(w, wpacked, static_cast<bf16_t*>(ws), C, C, &bw, s));
    GemmNTB g = gemm_ntb_conv3(x, B, H, W, C, bw, C, y, C);
    g.bias = bias;
    if (!res32) {
        g.res = res;
        return launch_gemm_nt_bf16(g, EB_RESID, s);
    }
    g.res32 = res32; g.C32 = y32;
    return launch_gemm_nt_bf16(g, EB_RESID32, s);
}

}  // namespace

// =====================================================================================================
extern "C" size_t dcpt_rcab_bf16_ws_bytes(int B, int H, int W, int C, int Cr) {
    if (!rcab_ok(B, H, W, C, Cr)) return 0;
    return rcab_layout(B, H, W, C, nullptr, 0, nullptr);
}
// (the stream form keeps the same intermediates: h, t, the column sums)
extern "C" size_t dcpt_rcab_bf16_res32_ws_bytes(int B, int H, int W, int C, int Cr) { return dcpt_rcab_bf16_ws_bytes(B, H, W, C, Cr); }

extern "C" int dcpt_rcab_fwd_bf16(const dcpt_rcab_params* p, const void* wpacked1, size_t wpacked1_bytes, const void* wpacked2,
                                  size_t wpacked2_bytes, const uint16_t* x, uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                                  int Cr, float res_scale, dcpt_stream_t stream) {
    return rcab_run("rcab_fwd_bf16", p, wpacked1, wpacked1_bytes, wpacked2, wpacked2_bytes, x, nullptr, y, nullptr, false, ws, ws_bytes, B, H, W, C, Cr,
                    res_scale, (hipStream_t)stream);
}

extern "C" int dcpt_rcab_fwd_bf16_res32(const dcpt_rcab_params* p, const void* wpacked1, size_t wpacked1_bytes, const void* wpacked2,
                                        size_t wpacked2_bytes, const float* x, const uint16_t* x_bf16, float* y, uint16_t* y_bf16, void* ws,
                                        size_t ws_bytes, int B, int H, int W, int C, int Cr, float res_scale, dcpt_stream_t stream) {
    return rcab_run("rcab_fwd_bf16_res32", p, wpacked1, wpacked1_bytes, wpacked2, wpacked2_bytes, x_bf16, x, y_bf16, y, true, ws, ws_bytes, B, H, W, C,
                    Cr, res_scale, (hipStream_t)stream);
}

// =====================================================================================================
extern "C" size_t dcpt_conv3x3_res_bf16_ws_bytes(int B, int H, int W, int C) {
    if (!conv3_ok(B, H, W, C, C)) return 0;
    return align_up((size_t)9 * C * C * sizeof(bf16_t), 256);
}
extern "C" size_t dcpt_conv3x3_res_bf16_res32_ws_bytes(int B, int H, int W, int C) { return dcpt_conv3x3_res_bf16_ws_bytes(B, H, W, C); }

extern "C" int dcpt_conv3x3_res_fwd_bf16(const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, const float* bias,
                                         const uint16_t* res, uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                                         dcpt_stream_t stream) {
    DCPT_CHECK_ARG(res && y, "conv3x3_res_fwd_bf16: null argument");
    return res_run("conv3x3_res_fwd_bf16", x, w, wpacked, wpacked_bytes, bias, res, nullptr, y, nullptr, ws, ws_bytes, B, H, W, C, (hipStream_t)stream);
}

extern "C" int dcpt_conv3x3_res_fwd_bf16_res32(const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, const float* bias,
                                               const float* res, float* y, uint16_t* y_bf16, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                                               dcpt_stream_t stream) {
    DCPT_CHECK_ARG(res, "conv3x3_res_fwd_bf16_res32: null argument");
    return res_run("conv3x3_res_fwd_bf16_res32", x, w, wpacked, wpacked_bytes, bias, nullptr, res, y_bf16, y, ws, ws_bytes, B, H, W, C,
                   (hipStream_t)stream);
}

// =====================================================================================================
extern "C" size_t dcpt_conv3x3_ps_bf16_ws_bytes(int B, int H, int W, int C, int r) {
    if (!ps_ok(B, H, W, C, r)) return 0;
    return align_up((size_t)9 * r * r * C * C * sizeof(bf16_t), 256);
}

extern "C" int dcpt_conv3x3_ps_fwd_bf16(const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, const float* bias,
                                        uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W, int C, int r, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(x && bias && y, "conv3x3_ps_fwd_bf16: null argument");
    DCPT_CHECK_ARG(ps_ok(B, H, W, C, r), "conv3x3_ps_fwd_bf16: B=%d H=%d W=%d C=%d r=%d (C a positive multiple of 8 up to 1024, r 2 or 3, one map inside the 32-bit windows)",
                   B, H, W, C, r);
    const int N = r * r * C;
    DCPT_CHECK_ARG(w || wpacked, "conv3x3_ps_fwd_bf16: null argument (weights)");
    DCPT_TRY(pk_check(wpacked, wpacked_bytes, C, N, 3, "conv3x3_ps_fwd_bf16"));
    const size_t need = dcpt_conv3x3_ps_bf16_ws_bytes(B, H, W, C, r);
    DCPT_CHECK_WS("conv3x3_ps_fwd_bf16", ws, ws_bytes, need);
    trace_tag("rcan_bf16.ps_fwd");
    const bf16_t* bw;
    DCPT_TRY(operand(w, wpacked, static_cast<bf16_t*>(ws), C, N, &bw, s));
    GemmNTB g = gemm_ntb_conv3(x, B, H, W, C, bw, N, y, N);
    g.bias = bias; g.psr = r;
    return launch_gemm_nt_bf16(g, EB_PSHUF, s);
}
