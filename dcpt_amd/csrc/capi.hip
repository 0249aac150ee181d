// C ABI entry points other than the NAFBlock pair (see include/dcpt_hip.h for the contract).
#include <stdarg.h>
#include <string.h>

#include "gemm.h"
#include "kernels.h"
#include "../../include/dcpt_hip.h"

static thread_local char g_err[512] = "";

void dcpt_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* dcpt_last_error(void) { return g_err; }
extern "C" int dcpt_abi_version(void) { return 16; }   // 16: one entry point per op, optional operands are NULL -- REMOVED: the *_packed and *_acc names (dcpt_conv_ln_fwd_bf16_packed, dcpt_conv_ln_bwd_acc / _acc_bf16 / _acc_bf16_packed, dcpt_conv1x1_pool_relu_fwd / _bwd_bf16_packed, dcpt_down2x2_bwd_acc / _acc_bf16, dcpt_nafblock_fwd / _bwd_bf16_packed) and dcpt_nchw_to_nhwc / dcpt_nhwc_to_nchw; CHANGED SIGNATURE: the plain names now take the full argument list of the removed form (dcpt_conv_ln_fwd_bf16, dcpt_conv_ln_bwd_bf16, dcpt_conv1x1_pool_relu_fwd_bf16 / _bwd_bf16, dcpt_nafblock_fwd_bf16 / _bwd_bf16: w/ the cached pack, NULL = pack in the call; dcpt_conv_ln_bwd, dcpt_conv_ln_bwd_bf16, dcpt_down2x2_bwd / _bf16: dx_add, NULL = none); 15: + dcpt_bottleneck_fwd_bf16 / _bwd_bf16 (the head's BottleneckBlock in one call, LayerNorms in GEMM epilogues), dcpt_trace_enable / dcpt_trace_read (launch trace for the tests); 14: + dcpt_conv_wpack_bf16_multi and the *_packed forms of the bf16 head's conv entry points (cached operand copies of the weights); 13: + dcpt_conv_ln_bwd_acc / _bf16 (the BottleneckBlock's shortcut gradient summed in the data-gradient GEMM), dcpt_down2x2_bwd_acc / _bf16 (the skip connection's gradient summed in the down layer's scatter epilogue); 12: + dcpt_adamw_step (multi-tensor AdamW); 11: + dcpt_mix_*_bf16 / dcpt_meanpool_fc_*_bf16 (the all-bf16 head without cast passes), dcpt_nafblock_bf16_fused_ffn may return 2 (chain kernel of the wide levels); 10: + dcpt_nafblock_wpack_bf16_multi; 9: + dcpt_conv1x1_wgrad_bf16 (grouped 256 x 256-tile weight-gradient GEMM + finisher); 8: + dcpt_nafblock_fused_ffn / dcpt_nafblock_bf16_fused_ffn (fused 1 x 1 chains of the narrowest level; saved tensors that become optional); 7: + per-block packed weights for the bf16 NAFBlock (dcpt_nafblock_wpack_bf16, *_packed); 6: + bf16-storage intro / ending / down / up layers; 5: + bf16-storage classifier-head groups; 4: + bf16-storage NAFBlock and casts; 3: + dcpt_allreduce_flat; 2: dcpt_nafblock_saved / mdta / gdfn saved structs carry the kept LN (and gate) tensors

// ---------------------------------------------------------------------------------------------
extern "C" int dcpt_ln2d_fwd(const float* x, const float* weight, const float* bias, float* y, float* mu, float* rstd,
                             int64_t M, int C, float eps, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && weight && bias && y && mu && rstd, "ln2d_fwd: null argument");
    return launch_ln_fwd(x, weight, bias, y, mu, rstd, M, C, eps, (hipStream_t)stream);
}

extern "C" size_t dcpt_ln2d_bwd_ws_bytes(int64_t M, int C) { return align_up((size_t)ln_bwd_num_blocks(M, C) * 3 * C * sizeof(float), 256); }

extern "C" int dcpt_ln2d_bwd(const float* dy, const float* x, const float* mu, const float* rstd, const float* weight,
                             float* dx, float* dweight, float* dbias, void* ws, size_t ws_bytes, int64_t M, int C,
                             dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(dy && x && mu && rstd && weight && dx, "ln2d_bwd: null argument");
    DCPT_CHECK_ARG(C > 0 && C % 4 == 0 && M > 0, "ln2d_bwd: bad shape");
    const int nblk = ln_bwd_num_blocks(M, C);
    DCPT_CHECK_WS("ln2d_bwd", ws, ws_bytes, dcpt_ln2d_bwd_ws_bytes(M, C));
    DCPT_TRY(launch_ln_bwd(dy, x, mu, rstd, weight, nullptr, dx, (float*)ws, nblk, M, C, s));
    DCPT_TRY(launch_colpart_reduce((float*)ws, nblk, 3, C, dweight, dbias, nullptr, s));
    return DCPT_OK;
}

// ---------------------------------------------------------------------------------------------
// intro-type conv: image NCHW (Cin small) -> features NHWC (Cout)
extern "C" int dcpt_conv3x3_in_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin,
                                   int Cout, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && w && y, "conv3x3_in_fwd: null argument");
    return launch_conv3x3_s2b(x, w, bias, y, B, H, W, Cin, Cout, 0, (hipStream_t)stream);
}

extern "C" size_t dcpt_conv3x3_in_bwd_ws_bytes(int B, int H, int W, int Cin, int Cout) {
    return align_up((size_t)conv3x3_wgrad_num_blocks(B, H, W, Cout) * (Cin * 9 + 1) * Cout * sizeof(float), 256);
}

extern "C" int dcpt_conv3x3_in_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias,
                                   void* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(dy && x && w && dw && dbias, "conv3x3_in_bwd: null argument");
    DCPT_CHECK_WS("conv3x3_in_bwd", ws, ws_bytes, dcpt_conv3x3_in_bwd_ws_bytes(B, H, W, Cin, Cout));
    const int nblk = conv3x3_wgrad_num_blocks(B, H, W, Cout);
    // dW[c][s][tap] = sum_p dy[p][c] * x[p+off][s];  db[c] = sum_p dy[p][c]
    DCPT_TRY(launch_conv3x3_wgrad(dy, x, (float*)ws, nblk, dw, dbias, B, H, W, Cin, Cout, 0, s));
    if (dx) DCPT_TRY(launch_conv3x3_b2s(dy, w, nullptr, nullptr, dx, B, H, W, Cin, Cout, 1, s));
    return DCPT_OK;
}

// ending-type conv: features NHWC (Cin) -> image NCHW (Cout small) (+ residual image)
extern "C" int dcpt_conv3x3_out_fwd(const float* x, const float* w, const float* bias, const float* res, float* y, int B,
                                    int H, int W, int Cin, int Cout, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && w && y, "conv3x3_out_fwd: null argument");
    return launch_conv3x3_b2s(x, w, bias, res, y, B, H, W, Cout, Cin, 0, (hipStream_t)stream);
}

extern "C" size_t dcpt_conv3x3_out_bwd_ws_bytes(int B, int H, int W, int Cin, int Cout) {
    return align_up((size_t)conv3x3_wgrad_num_blocks(B, H, W, Cin) * (Cout * 9 + 1) * Cin * sizeof(float), 256) +
           align_up((size_t)Cout * 128 * sizeof(float), 256);
}

extern "C" int dcpt_conv3x3_out_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias,
                                    void* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(dy && x && w && dx && dw && dbias, "conv3x3_out_bwd: null argument");
    DCPT_CHECK_WS("conv3x3_out_bwd", ws, ws_bytes, dcpt_conv3x3_out_bwd_ws_bytes(B, H, W, Cin, Cout));
    // dx[p][c] = sum_{s,tap} dy[p-off][s] * w[s][c][tap]
    DCPT_TRY(launch_conv3x3_s2b(dy, w, nullptr, dx, B, H, W, Cout, Cin, 1, s));
    // dW[s][c][tap] = sum_p dy[p][s]*x[p+off][c] = sum_p' x[p'][c]*dy[p'-off][s]  (flipped-tap form)
    const int nblk = conv3x3_wgrad_num_blocks(B, H, W, Cin);
    DCPT_TRY(launch_conv3x3_wgrad(x, dy, (float*)ws, nblk, dw, nullptr, B, H, W, Cout, Cin, 1, s));
    float* cspart = (float*)((char*)ws + align_up((size_t)nblk * (Cout * 9 + 1) * Cin * sizeof(float), 256));
    DCPT_TRY(launch_nchw_channel_sum(dy, cspart, dbias, B, Cout, H * W, s));
    return DCPT_OK;
}

// ---------------------------------------------------------------------------------------------
// down: x [B][H][W][C] -> y [B][H/2][W/2][2C]
namespace {
struct DownWs {
    float* wp;      // fwd: packed [2C][4C]; bwd: packed-transposed [4C][2C]
    float* slab;
    float* colsum;
    int splits;
    int64_t rps;
};
size_t down_layout(int B, int H, int W, int C, int backward, void* base, size_t bytes, DownWs* out) {
    WsAlloc a(base, bytes);
    DownWs w{};
    w.wp = a.get<float>((size_t)8 * C * C);
    if (backward) {
        const int64_t Mc = (int64_t)B * (H / 2) * (W / 2);
        gemm_tn_plan(Mc, 2 * C, 4 * C, &w.splits, &w.rps);
        w.slab = a.get<float>((size_t)w.splits * 8 * C * C);
        w.colsum = a.get<float>((size_t)w.splits * gemm_tn_tiles_k(2 * C, 4 * C) * 2 * C);
    }
    if (out) *out = w;
    return a.off;
}
}  // namespace

extern "C" size_t dcpt_down2x2_ws_bytes(int B, int H, int W, int C, int backward) {
    return down_layout(B, H, W, C, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_down2x2_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B,
                                int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(x && w && y, "down2x2_fwd: null argument");
    DCPT_CHECK_ARG(H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "down2x2_fwd: H=%d W=%d must be even, C=%d %% 4", H, W, C);
    DownWs d;
    const size_t need = down_layout(B, H, W, C, 0, ws, ws_bytes, &d);
    DCPT_CHECK_WS("down2x2_fwd", ws, ws_bytes, need);
    DCPT_TRY(launch_wpack(w, d.wp, nullptr, 2 * C, 4 * C, WP_DOWN, s));
    GemmNT g{};
    g.M = (int64_t)B * (H / 2) * (W / 2);
    g.A = x; g.K = 4 * C; g.gH = H / 2; g.gW = W / 2; g.gC = C;
    g.Bw = d.wp; g.N = 2 * C; g.C = y; g.ldc = 2 * C; g.bias = bias;
    return launch_gemm_nt(g, A_GATHER, E_BIAS, s);
}

extern "C" int dcpt_down2x2_bwd(const float* dy, const float* x, const float* w, const float* dx_add, float* dx, float* dw, float* dbias,
                                void* ws, size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(dy && x && w && dx && dw && dbias, "down2x2_bwd: null argument");
    DCPT_CHECK_ARG(H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "down2x2_bwd: bad shape");
    DownWs d;
    const size_t need = down_layout(B, H, W, C, 1, ws, ws_bytes, &d);
    DCPT_CHECK_WS("down2x2_bwd", ws, ws_bytes, need);
    const int64_t Mc = (int64_t)B * (H / 2) * (W / 2);
    // dx (fine) = scatter( dy [Mc][2C] x Wp^T )  ;  Bw [N=4C][K=2C]
    DCPT_TRY(launch_wpack(w, d.wp, nullptr, 2 * C, 4 * C, WP_DOWN_T, s));
    GemmNT g{};
    g.M = Mc; g.A = dy; g.lda = 2 * C; g.K = 2 * C; g.Bw = d.wp; g.N = 4 * C; g.C = dx;
    g.gH = H / 2; g.gW = W / 2; g.gC = C;
    g.res = dx_add;   // (the encoder output's second consumer is the skip connection: its gradient joins in the scatter epilogue)
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, dx_add ? E_SCATTER_ADD : E_SCATTER, s));
    // dW packed [2C][4C] = sum_m dy[m][oc] * gather(x)[m][k']
    GemmTN t{};
    t.M = Mc; t.X = dy; t.ldx = 2 * C; t.N = 2 * C; t.Y = x; t.K = 4 * C;
    t.gH = H / 2; t.gW = W / 2; t.gC = C;
    t.slab = d.slab; t.colsum = d.colsum; t.splits = d.splits; t.rows_per_split = d.rps;
    DCPT_TRY(launch_gemm_tn(t, A_PLAIN, A_GATHER, s));
    DCPT_TRY(launch_wgrad_reduce(d.slab, d.colsum, d.splits, d.splits * gemm_tn_tiles_k(2 * C, 4 * C), 2 * C, 4 * C, nullptr, nullptr,
                                 nullptr, dw, nullptr, dbias, WR_DOWN, s));
    return DCPT_OK;
}

// ---------------------------------------------------------------------------------------------
// up: x [B][H][W][C] -> y [B][2H][2W][C/2] = PixelShuffle2(conv1x1(x)) + skip
namespace {
struct UpWs {
    float* wp;  // packed [2C][C] (fwd) or [C][2C] (bwd)
    float* slab;
    int splits;
    int64_t rps;
};
size_t up_layout(int B, int H, int W, int C, int backward, void* base, size_t bytes, UpWs* out) {
    WsAlloc a(base, bytes);
    UpWs w{};
    w.wp = a.get<float>((size_t)2 * C * C);
    if (backward) {
        gemm_tn_plan((int64_t)B * H * W, 2 * C, C, &w.splits, &w.rps);
        w.slab = a.get<float>((size_t)w.splits * 2 * C * C);
    }
    if (out) *out = w;
    return a.off;
}
}  // namespace

extern "C" size_t dcpt_up_ps_ws_bytes(int B, int H, int W, int C, int backward) {
    return up_layout(B, H, W, C, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_up_ps_fwd(const float* x, const float* w, const float* skip, float* y, void* ws, size_t ws_bytes, int B,
                              int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(x && w && y, "up_ps_fwd: null argument");
    DCPT_CHECK_ARG(C % 8 == 0, "up_ps_fwd: C=%d must be a multiple of 8", C);
    UpWs u;
    const size_t need = up_layout(B, H, W, C, 0, ws, ws_bytes, &u);
    DCPT_CHECK_WS("up_ps_fwd", ws, ws_bytes, need);
    DCPT_TRY(launch_wpack(w, u.wp, nullptr, 2 * C, C, WP_UP, s));
    GemmNT g{};
    g.M = (int64_t)B * H * W; g.A = x; g.lda = C; g.K = C; g.Bw = u.wp; g.N = 2 * C; g.C = y;
    g.gH = H; g.gW = W; g.gC = C / 2; g.res = skip;
    return launch_gemm_nt(g, A_PLAIN, skip ? E_SCATTER_ADD : E_SCATTER, s);
}

extern "C" int dcpt_up_ps_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, void* ws, size_t ws_bytes,
                              int B, int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(dy && x && w && dx && dw, "up_ps_bwd: null argument");
    DCPT_CHECK_ARG(C % 8 == 0, "up_ps_bwd: C=%d must be a multiple of 8", C);
    UpWs u;
    const size_t need = up_layout(B, H, W, C, 1, ws, ws_bytes, &u);
    DCPT_CHECK_WS("up_ps_bwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    // dx[m][ic] = sum_n' gather(dy)[m][n'] * Wp[n'][ic]  ->  Bw [N=C][K=2C] = Wp^T
    DCPT_TRY(launch_wpack(w, u.wp, nullptr, 2 * C, C, WP_UP_T, s));
    GemmNT g{};
    g.M = M; g.A = dy; g.K = 2 * C; g.gH = H; g.gW = W; g.gC = C / 2; g.Bw = u.wp; g.N = C; g.C = dx; g.ldc = C;
    DCPT_TRY(launch_gemm_nt(g, A_GATHER, E_PLAIN, s));
    // dW packed [2C][C] = sum_m gather(dy)[m][n'] * x[m][ic]
    GemmTN t{};
    t.M = M; t.X = dy; t.N = 2 * C; t.Y = x; t.ldy = C; t.K = C; t.gH = H; t.gW = W; t.gC = C / 2;
    t.slab = u.slab; t.colsum = nullptr; t.splits = u.splits; t.rows_per_split = u.rps;
    DCPT_TRY(launch_gemm_tn(t, A_GATHER, A_PLAIN, s));
    DCPT_TRY(launch_wgrad_reduce(u.slab, nullptr, u.splits, 0, 2 * C, C, nullptr, nullptr, nullptr, dw, nullptr, nullptr, WR_UP, s));
    return DCPT_OK;
}

// ---------------------------------------------------------------------------------------------
namespace {
__global__ void fused_bias_act_kernel(const float* __restrict__ x, const float* __restrict__ bias, const float* __restrict__ ref,
                                      float* __restrict__ y, int64_t n, int size_b, int64_t step_b, int act, int grad,
                                      float alpha, float scale) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float v = x[i];
        if (bias) v += bias[(i / step_b) % size_b];
        const float r = ref ? ref[i] : 0.f;
        float o;
        if (act == 3) {  // leaky relu
            if (grad == 0) o = (v > 0.f) ? v : v * alpha;
            else if (grad == 1) o = (r > 0.f) ? v : v * alpha;
            else o = 0.f;
        } else {  // linear
            o = (grad == 2) ? 0.f : v;
        }
        y[i] = o * scale;
    }
}
}  // namespace

extern "C" int dcpt_fused_bias_act(const float* x, const float* bias, const float* ref, float* y, int64_t n, int size_b,
                                   int64_t step_b, int act, int grad, float alpha, float scale, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && y && n >= 0, "fused_bias_act: null argument");
    DCPT_CHECK_ARG(act == 1 || act == 3, "fused_bias_act: act=%d (1 linear, 3 leaky relu)", act);
    DCPT_CHECK_ARG(!bias || (size_b > 0 && step_b > 0), "fused_bias_act: bad bias geometry");
    if (n == 0) return DCPT_OK;
    int64_t nb = cdiv64(n, 256);
    if (nb > 4096) nb = 4096;
    fused_bias_act_kernel<<<dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream>>>(x, bias, ref, y, n, size_b, step_b, act,
                                                                                     grad, alpha, scale);
    DCPT_CHECK_LAUNCH("fused_bias_act");
    return DCPT_OK;
}

// ---------------------------------------------------------------------------------------------
// validation metrics (metrics.hip)
namespace {
struct MetricWs {
    double* ssim_part;
    void* sse_part;
};
// The one check of every metric-shaped entry point (imgmetric, msssim, ssim_matlab, imgrange, ssim_loss): 0 on success, else the message
// that names what is wrong with the shape / flags, "<op>: ...".  `taken` are the flags the op accepts and `taken_text` what the message
// says about them; `window` names what needs a cropped image of 11 x 11 (null: any size will do); `levels` is MS-SSIM's count (null: the
// op has none).  The message lives until this thread's next call.
const char* metric_check(const char* op, int taken, const char* taken_text, const char* window, const int* levels, int B, int C, int H, int W,
                         int crop, int flags) {
    static thread_local char msg[160];
    char text[128];
    const int64_t Hc = (int64_t)H - 2 * (int64_t)crop, Wc = (int64_t)W - 2 * (int64_t)crop;
    if (B <= 0 || H <= 0 || W <= 0) snprintf(text, sizeof text, "bad shape");
    else if (C != 1 && C != 3) snprintf(text, sizeof text, "C must be 1 or 3");
    else if (crop < 0) snprintf(text, sizeof text, "crop_border must be >= 0");
    else if (flags & ~taken) snprintf(text, sizeof text, "unknown flag (%s)", taken_text);
    else if (Hc <= 0 || Wc <= 0) snprintf(text, sizeof text, "nothing left after the crop");
    else if (window && (Hc < 11 || Wc < 11)) snprintf(text, sizeof text, "%s needs a cropped image of at least 11 x 11", window);
    else if (levels && (*levels < 1 || *levels > MSSSIM_MAX_LEVELS)) snprintf(text, sizeof text, "levels must be 1 .. %d", MSSSIM_MAX_LEVELS);
    // (the grid's y extent; C, not C': one bound for both luma settings)
    else if ((int64_t)B * C * (levels ? *levels : 1) > 65535) snprintf(text, sizeof text, "B * C%s above 65535", levels ? " * levels" : "");
    else return nullptr;
    snprintf(msg, sizeof msg, "%s: %s", op, text);
    return msg;
}
const char* imgmetric_check(int B, int C, int H, int W, int crop, int flags) {
    return metric_check("imgmetric", DCPT_METRIC_Y | DCPT_METRIC_SSIM | DCPT_METRIC_RANGE1, "image_range is 255, or 1 with DCPT_METRIC_RANGE1",
                        (flags & DCPT_METRIC_SSIM) ? "SSIM" : nullptr, nullptr, B, C, H, W, crop, flags);
}
size_t metric_layout(int B, int C, int H, int W, int crop, int flags, void* base, size_t bytes, MetricWs* out) {
    WsAlloc a(base, bytes);
    const int Cp = ((flags & DCPT_METRIC_Y) && C == 3) ? 1 : C;
    const size_t n = (size_t)B * Cp * metric_num_tiles(H - 2 * crop, W - 2 * crop);
    MetricWs w{};
    w.ssim_part = a.get<double>(n);
    w.sse_part = a.get<uint64_t>(n);
    if (out) *out = w;
    return a.off;
}
}  // namespace

extern "C" size_t dcpt_imgmetric_ws_bytes(int B, int C, int H, int W, int crop_border, int flags) {
    if (imgmetric_check(B, C, H, W, crop_border, flags)) return 0;
    return metric_layout(B, C, H, W, crop_border, flags, nullptr, 0, nullptr);
}

extern "C" int dcpt_imgmetric(const float* img, const float* img2, void* sse_out, double* ssim_out, void* ws, size_t ws_bytes, int B, int C,
                              int H, int W, int crop_border, int flags, dcpt_stream_t stream) {
    const int want_ssim = (flags & DCPT_METRIC_SSIM) != 0;
    DCPT_CHECK_ARG(img && img2 && sse_out && (ssim_out || !want_ssim), "imgmetric: null argument");
    const char* bad = imgmetric_check(B, C, H, W, crop_border, flags);
    DCPT_CHECK_ARG(!bad, "%s (B=%d C=%d H=%d W=%d crop_border=%d flags=0x%x)", bad, B, C, H, W, crop_border, flags);
    MetricWs m;
    const size_t need = metric_layout(B, C, H, W, crop_border, flags, ws, ws_bytes, &m);
    DCPT_CHECK_WS("imgmetric", ws, ws_bytes, need);
    return launch_imgmetric(img, img2, sse_out, ssim_out, m.ssim_part, m.sse_part, B, C, H, W, crop_border, (flags & DCPT_METRIC_Y) != 0,
                            (flags & DCPT_METRIC_RANGE1) ? 1 : 255, want_ssim, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// MS-SSIM, MATLAB SSIM and the NRMSE range (metrics_ms.hip)
namespace {
enum { MS_MSSSIM, MS_MATLAB, MS_RANGE };
const char* msmetric_check(int kind, int B, int C, int H, int W, int crop, int flags, int levels) {
    static const char* const op[3] = {"msssim", "ssim_matlab", "imgrange"};
    const bool ms = kind == MS_MSSSIM;
    return metric_check(op[kind], DCPT_METRIC_Y | DCPT_METRIC_RANGE1, "DCPT_METRIC_Y and DCPT_METRIC_RANGE1 are taken", ms ? "MS-SSIM" : nullptr,
                        ms ? &levels : nullptr, B, C, H, W, crop, flags);
}
size_t msmetric_part_doubles(int kind, int B, int C, int H, int W, int crop, int flags, int levels) {
    const int Cp = ((flags & DCPT_METRIC_Y) && C == 3) ? 1 : C;
    const int Hc = H - 2 * crop, Wc = W - 2 * crop;
    if (kind == MS_MSSSIM) return (size_t)B * levels * metric_num_tiles(Hc, Wc) * 2;
    if (kind == MS_MATLAB) return (size_t)B * Cp * ssim_matlab_num_tiles(Hc, Wc);
    return (size_t)B * (size_t)imgrange_num_chunks(Cp, Hc, Wc) * 2;
}
size_t msmetric_layout(int kind, int B, int C, int H, int W, int crop, int flags, int levels, void* base, size_t bytes, double** part) {
    WsAlloc a(base, bytes);
    double* p = a.get<double>(msmetric_part_doubles(kind, B, C, H, W, crop, flags, levels));
    if (part) *part = p;
    return a.off;
}
}  // namespace

extern "C" size_t dcpt_msssim_ws_bytes(int B, int C, int H, int W, int crop_border, int flags, int levels) {
    if (msmetric_check(MS_MSSSIM, B, C, H, W, crop_border, flags, levels)) return 0;
    return msmetric_layout(MS_MSSSIM, B, C, H, W, crop_border, flags, levels, nullptr, 0, nullptr);
}

extern "C" int dcpt_msssim(const float* img, const float* img2, double* out, void* ws, size_t ws_bytes, int B, int C, int H, int W,
                           int crop_border, int flags, int levels, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(img && img2 && out, "msssim: null argument");
    const char* bad = msmetric_check(MS_MSSSIM, B, C, H, W, crop_border, flags, levels);
    DCPT_CHECK_ARG(!bad, "%s (B=%d C=%d H=%d W=%d crop_border=%d flags=0x%x levels=%d)", bad, B, C, H, W, crop_border, flags, levels);
    double* part;
    const size_t need = msmetric_layout(MS_MSSSIM, B, C, H, W, crop_border, flags, levels, ws, ws_bytes, &part);
    DCPT_CHECK_WS("msssim", ws, ws_bytes, need);
    return launch_msssim(img, img2, out, part, B, C, H, W, crop_border, (flags & DCPT_METRIC_Y) != 0, (flags & DCPT_METRIC_RANGE1) ? 1 : 255,
                         levels, (hipStream_t)stream);
}

extern "C" size_t dcpt_ssim_matlab_ws_bytes(int B, int C, int H, int W, int crop_border, int flags) {
    if (msmetric_check(MS_MATLAB, B, C, H, W, crop_border, flags, 1)) return 0;
    return msmetric_layout(MS_MATLAB, B, C, H, W, crop_border, flags, 1, nullptr, 0, nullptr);
}

extern "C" int dcpt_ssim_matlab(const float* img, const float* img2, double* out, void* ws, size_t ws_bytes, int B, int C, int H, int W,
                                int crop_border, int flags, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(img && img2 && out, "ssim_matlab: null argument");
    const char* bad = msmetric_check(MS_MATLAB, B, C, H, W, crop_border, flags, 1);
    DCPT_CHECK_ARG(!bad, "%s (B=%d C=%d H=%d W=%d crop_border=%d flags=0x%x)", bad, B, C, H, W, crop_border, flags);
    double* part;
    const size_t need = msmetric_layout(MS_MATLAB, B, C, H, W, crop_border, flags, 1, ws, ws_bytes, &part);
    DCPT_CHECK_WS("ssim_matlab", ws, ws_bytes, need);
    return launch_ssim_matlab(img, img2, out, part, B, C, H, W, crop_border, (flags & DCPT_METRIC_Y) != 0,
                              (flags & DCPT_METRIC_RANGE1) ? 1 : 255, (hipStream_t)stream);
}

extern "C" size_t dcpt_imgrange_ws_bytes(int B, int C, int H, int W, int crop_border, int flags) {
    if (msmetric_check(MS_RANGE, B, C, H, W, crop_border, flags, 1)) return 0;
    return msmetric_layout(MS_RANGE, B, C, H, W, crop_border, flags, 1, nullptr, 0, nullptr);
}

extern "C" int dcpt_imgrange(const float* img, double* out, void* ws, size_t ws_bytes, int B, int C, int H, int W, int crop_border, int flags,
                             dcpt_stream_t stream) {
    DCPT_CHECK_ARG(img && out, "imgrange: null argument");
    const char* bad = msmetric_check(MS_RANGE, B, C, H, W, crop_border, flags, 1);
    DCPT_CHECK_ARG(!bad, "%s (B=%d C=%d H=%d W=%d crop_border=%d flags=0x%x)", bad, B, C, H, W, crop_border, flags);
    double* part;
    const size_t need = msmetric_layout(MS_RANGE, B, C, H, W, crop_border, flags, 1, ws, ws_bytes, &part);
    DCPT_CHECK_WS("imgrange", ws, ws_bytes, need);
    return launch_imgrange(img, out, part, B, C, H, W, crop_border, (flags & DCPT_METRIC_Y) != 0, (flags & DCPT_METRIC_RANGE1) ? 1 : 255,
                           (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// SSIM as a training loss (ssim_loss.hip)
namespace {
struct SsimLossWs {
    double* part;     // [B * C'][tiles]
    double* planes;   // [chunk images * C'][3][Hm][Wm] (backward)
};
const char* ssim_loss_check(int B, int C, int H, int W, int crop, int flags) {
    return metric_check("ssim_loss", DCPT_METRIC_Y, "only DCPT_METRIC_Y is taken", "SSIM", nullptr, B, C, H, W, crop, flags);
}
size_t ssim_loss_layout(int B, int C, int H, int W, int crop, int flags, int backward, void* base, size_t bytes, SsimLossWs* out) {
    WsAlloc a(base, bytes);
    const int Cp = ((flags & DCPT_METRIC_Y) && C == 3) ? 1 : C;
    const int Hc = H - 2 * crop, Wc = W - 2 * crop;
    SsimLossWs w{};
    w.part = a.get<double>((size_t)B * Cp * ssim_loss_num_tiles(Hc, Wc));
    if (backward) w.planes = (double*)a.get<char>((size_t)ssim_loss_chunk_images(B, Cp, Hc, Wc) * ssim_loss_plane_bytes(Cp, Hc, Wc));
    if (out) *out = w;
    return a.off;
}
}  // namespace

extern "C" size_t dcpt_ssim_loss_ws_bytes(int B, int C, int H, int W, int crop_border, int flags, int backward) {
    if (ssim_loss_check(B, C, H, W, crop_border, flags)) return 0;
    return ssim_loss_layout(B, C, H, W, crop_border, flags, backward != 0, nullptr, 0, nullptr);
}

extern "C" int dcpt_ssim_loss_fwd(const float* pred, const float* target, double* ssim_sum, void* ws, size_t ws_bytes, int B, int C, int H, int W,
                                  int crop_border, int flags, double image_range, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(pred && target && ssim_sum, "ssim_loss_fwd: null argument");
    const char* bad = ssim_loss_check(B, C, H, W, crop_border, flags);
    DCPT_CHECK_ARG(!bad, "%s (B=%d C=%d H=%d W=%d crop_border=%d flags=0x%x)", bad, B, C, H, W, crop_border, flags);
    DCPT_CHECK_ARG(image_range > 0, "ssim_loss: image_range must be > 0 (got %g)", image_range);
    SsimLossWs m;
    const size_t need = ssim_loss_layout(B, C, H, W, crop_border, flags, 0, ws, ws_bytes, &m);
    DCPT_CHECK_WS("ssim_loss_fwd", ws, ws_bytes, need);
    return launch_ssim_loss_fwd(pred, target, ssim_sum, m.part, B, C, H, W, crop_border, (flags & DCPT_METRIC_Y) != 0, image_range,
                                (hipStream_t)stream);
}

extern "C" int dcpt_ssim_loss_bwd(const float* pred, const float* target, const double* gscale, float* dpred, void* ws, size_t ws_bytes, int B,
                                  int C, int H, int W, int crop_border, int flags, double image_range, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(pred && target && gscale && dpred, "ssim_loss_bwd: null argument");
    const char* bad = ssim_loss_check(B, C, H, W, crop_border, flags);
    DCPT_CHECK_ARG(!bad, "%s (B=%d C=%d H=%d W=%d crop_border=%d flags=0x%x)", bad, B, C, H, W, crop_border, flags);
    DCPT_CHECK_ARG(image_range > 0, "ssim_loss: image_range must be > 0 (got %g)", image_range);
    SsimLossWs m;
    const size_t need = ssim_loss_layout(B, C, H, W, crop_border, flags, 1, ws, ws_bytes, &m);
    DCPT_CHECK_WS("ssim_loss_bwd", ws, ws_bytes, need);
    return launch_ssim_loss_bwd(pred, target, gscale, dpred, m.planes, B, C, H, W, crop_border, (flags & DCPT_METRIC_Y) != 0, image_range,
                                (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// The LDL artifact-weight map (ldl.hip)
namespace {
// 0 on success; the message names what is wrong with the shape
const char* ldl_check(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return "ldl_weight: bad shape";
    if ((int64_t)B * C * H * W < 2) return "ldl_weight: the std over the map needs B * C * H * W >= 2";
    if (H < 4 || W < 4) return "ldl_weight: reflect padding by 3 needs H >= 4 and W >= 4";
    if ((int64_t)B * C > 65535) return "ldl_weight: B * C above 65535";
    if ((int64_t)H * W > ((int64_t)1 << 30)) return "ldl_weight: a plane above 2^30 pixels";
    return nullptr;
}
size_t ldl_layout(int B, int C, int H, int W, int backward, void* base, size_t bytes, LdlWs* out) {
    WsAlloc a(base, bytes);
    const size_t N = (size_t)B * C * H * W;
    LdlWs w{};
    w.scal = a.get<double>(8);
    w.part = a.get<double>(2 * (size_t)ldl_num_partials(B, C, H, W));
    w.u = a.get<double>(N);
    w.mu = a.get<double>(N);
    if (backward) {
        w.gv = a.get<double>(N);
        w.gvmu = a.get<double>(N);
    }
    if (out) *out = w;
    return a.off;
}
}  // namespace

extern "C" size_t dcpt_ldl_weight_ws_bytes(int B, int C, int H, int W, int backward) {
    if (ldl_check(B, C, H, W)) return 0;
    return ldl_layout(B, C, H, W, backward != 0, nullptr, 0, nullptr);
}

extern "C" int dcpt_ldl_weight_fwd(const float* gt, const float* out, float* w, void* ws, size_t ws_bytes, int B, int C, int H, int W,
                                   dcpt_stream_t stream) {
    DCPT_CHECK_ARG(gt && out && w, "ldl_weight_fwd: null argument");
    const char* bad = ldl_check(B, C, H, W);
    DCPT_CHECK_ARG(!bad, "%s (B=%d C=%d H=%d W=%d)", bad, B, C, H, W);
    LdlWs m;
    const size_t need = ldl_layout(B, C, H, W, 0, ws, ws_bytes, &m);
    DCPT_CHECK_WS("ldl_weight_fwd", ws, ws_bytes, need);
    return launch_ldl_weight_fwd(gt, out, w, m, B, C, H, W, (hipStream_t)stream);
}

extern "C" int dcpt_ldl_weight_bwd(const float* gt, const float* out, const float* gw, float* dout, void* ws, size_t ws_bytes, int B, int C,
                                   int H, int W, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(gt && out && gw && dout, "ldl_weight_bwd: null argument");
    const char* bad = ldl_check(B, C, H, W);
    DCPT_CHECK_ARG(!bad, "%s (B=%d C=%d H=%d W=%d)", bad, B, C, H, W);
    LdlWs m;
    const size_t need = ldl_layout(B, C, H, W, 1, ws, ws_bytes, &m);
    DCPT_CHECK_WS("ldl_weight_bwd", ws, ws_bytes, need);
    return launch_ldl_weight_bwd(gt, out, gw, dout, m, B, C, H, W, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// The DiffJPEG round trip (jpeg.hip)
extern "C" int dcpt_diffjpeg_fwd(const float* x, const float* quality, float* y, int B, int C, int H, int W, int flags, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && quality && y, "diffjpeg_fwd: null argument");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0, "diffjpeg_fwd: bad shape (B=%d C=%d H=%d W=%d)", B, C, H, W);
    DCPT_CHECK_ARG(C == 1 || C == 3, "diffjpeg_fwd: C must be 1 or 3 (got %d)", C);
    DCPT_CHECK_ARG((flags & ~(DCPT_JPEG_DIFF_ROUND | DCPT_JPEG_UINT8_IO)) == 0, "diffjpeg_fwd: unknown flags 0x%x", flags);
    DCPT_CHECK_ARG(B <= 65535, "diffjpeg_fwd: B above 65535 (got %d)", B);
    DCPT_CHECK_ARG((int64_t)H * W <= ((int64_t)1 << 30), "diffjpeg_fwd: a plane above 2^30 pixels (H=%d W=%d)", H, W);
    return launch_diffjpeg_fwd(x, quality, y, B, C, H, W, flags, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// MATLAB-bicubic resize and the NIQE pixel work (niqe.hip)
namespace {
const char* imresize_check(int P, int H, int W, int Ho, int Wo, int Kh, int Kw) {
    if (P <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return "imresize: bad shape";
    if (Kh <= 0 || Kw <= 0 || Kh > 4096 || Kw > 4096) return "imresize: the tap count per axis must lie in 1..4096";
    if ((int64_t)H * W > ((int64_t)1 << 30) || (int64_t)Ho * Wo > ((int64_t)1 << 30) || (int64_t)Ho * W > ((int64_t)1 << 30))
        return "imresize: a plane above 2^30 pixels";
    if ((int64_t)P * Ho * W > ((int64_t)1 << 36) || (int64_t)P * Ho * Wo > ((int64_t)1 << 36)) return "imresize: above 2^36 elements";
    return nullptr;
}
}  // namespace

extern "C" size_t dcpt_imresize_ws_bytes(int P, int H, int W, int Ho, int Wo, int Kh, int Kw) {
    if (imresize_check(P, H, W, Ho, Wo, Kh, Kw)) return 0;
    return align_up((size_t)P * Ho * W * sizeof(double), 256);
}

extern "C" int dcpt_imresize_fwd(const void* x, void* y, const int* first_h, const double* w_h, const int* first_w, const double* w_w, void* ws,
                                 size_t ws_bytes, int P, int H, int W, int Ho, int Wo, int Kh, int Kw, int64_t plane_stride,
                                 int64_t row_stride, int flags, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && y && first_h && w_h && first_w && w_w, "imresize_fwd: null argument");
    const char* bad = imresize_check(P, H, W, Ho, Wo, Kh, Kw);
    DCPT_CHECK_ARG(!bad, "%s (P=%d H=%d W=%d Ho=%d Wo=%d Kh=%d Kw=%d)", bad, P, H, W, Ho, Wo, Kh, Kw);
    DCPT_CHECK_ARG((flags & ~(DCPT_IMRESIZE_X_F64 | DCPT_IMRESIZE_Y_F64 | DCPT_IMRESIZE_QUANT8)) == 0, "imresize_fwd: unknown flags 0x%x", flags);
    DCPT_CHECK_ARG(!((flags & DCPT_IMRESIZE_QUANT8) && (flags & DCPT_IMRESIZE_X_F64)), "imresize_fwd: DCPT_IMRESIZE_QUANT8 takes an fp32 source");
    DCPT_CHECK_ARG(row_stride >= W && plane_stride >= (int64_t)(H - 1) * row_stride + W,
                   "imresize_fwd: strides overlap (plane_stride=%lld row_stride=%lld H=%d W=%d)", (long long)plane_stride, (long long)row_stride,
                   H, W);
    DCPT_CHECK_WS("imresize_fwd", ws, ws_bytes, dcpt_imresize_ws_bytes(P, H, W, Ho, Wo, Kh, Kw));
    return launch_imresize_fwd(x, y, first_h, w_h, first_w, w_w, (double*)ws, P, H, W, Ho, Wo, Kh, Kw, plane_stride, row_stride,
                               (flags & DCPT_IMRESIZE_X_F64) != 0, (flags & DCPT_IMRESIZE_Y_F64) != 0, (flags & DCPT_IMRESIZE_QUANT8) != 0,
                               (hipStream_t)stream);
}

extern "C" int dcpt_niqe_mscn_fwd(const void* x, double* n, int P, int H, int W, int crop_border, int scale, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && n, "niqe_mscn_fwd: null argument");
    DCPT_CHECK_ARG(P > 0 && H > 0 && W > 0 && crop_border >= 0, "niqe_mscn_fwd: bad shape (P=%d H=%d W=%d crop_border=%d)", P, H, W, crop_border);
    DCPT_CHECK_ARG(scale == 1 || scale == 2, "niqe_mscn_fwd: scale must be 1 or 2 (got %d)", scale);
    DCPT_CHECK_ARG(P <= 65535, "niqe_mscn_fwd: above 65535 planes (got %d)", P);
    DCPT_CHECK_ARG((int64_t)H * W <= ((int64_t)1 << 30), "niqe_mscn_fwd: a plane above 2^30 pixels (H=%d W=%d)", H, W);
    int Hc = H, Wc = W;
    if (scale == 1) {
        DCPT_CHECK_ARG((int64_t)2 * crop_border < H && (int64_t)2 * crop_border < W, "niqe_mscn_fwd: nothing left after the crop (H=%d W=%d crop_border=%d)",
                       H, W, crop_border);
        Hc = (H - 2 * crop_border) / 96 * 96;
        Wc = (W - 2 * crop_border) / 96 * 96;
        DCPT_CHECK_ARG(Hc > 0 && Wc > 0, "niqe_mscn_fwd: no whole 96 x 96 block in the cropped plane (H=%d W=%d crop_border=%d)", H, W, crop_border);
    } else {
        DCPT_CHECK_ARG(crop_border == 0 && H % 48 == 0 && W % 48 == 0,
                       "niqe_mscn_fwd: scale 2 takes whole 48 x 48 blocks and no crop (H=%d W=%d crop_border=%d)", H, W, crop_border);
    }
    return launch_niqe_mscn_fwd(x, n, P, H, W, crop_border, Hc, Wc, scale, (hipStream_t)stream);
}

extern "C" int dcpt_niqe_block_stats_fwd(const double* n, double* stats, int P, int H, int W, int block, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(n && stats, "niqe_block_stats_fwd: null argument");
    DCPT_CHECK_ARG(block == 96 || block == 48, "niqe_block_stats_fwd: block must be 96 or 48 (got %d)", block);
    DCPT_CHECK_ARG(P > 0 && H > 0 && W > 0 && H % block == 0 && W % block == 0,
                   "niqe_block_stats_fwd: the plane must hold whole blocks (P=%d H=%d W=%d block=%d)", P, H, W, block);
    DCPT_CHECK_ARG(P <= 65535, "niqe_block_stats_fwd: above 65535 planes (got %d)", P);
    DCPT_CHECK_ARG((int64_t)H * W <= ((int64_t)1 << 30), "niqe_block_stats_fwd: a plane above 2^30 pixels (H=%d W=%d)", H, W);
    return launch_niqe_block_stats_fwd(n, stats, P, H, W, block, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// The demosaic and the line-mask inpainting degradation (degrade.hip)
extern "C" int dcpt_demosaic_fwd(const float* x, float* y, int B, int C, int H, int W, int flags, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && y, "demosaic_fwd: null argument");
    DCPT_CHECK_ARG(x != y, "demosaic_fwd: x and y must be different buffers (a pixel reads its neighbours)");
    DCPT_CHECK_ARG(C == 1 || C == 3, "demosaic_fwd: C must be 1 or 3 (got %d)", C);
    DCPT_CHECK_ARG(H >= 3 && W >= 3, "demosaic_fwd: H and W must be at least 3 (H=%d W=%d)", H, W);
    DCPT_CHECK_ARG(B >= 1 && B <= 65535, "demosaic_fwd: B outside 1..65535 (got %d)", B);
    DCPT_CHECK_ARG((int64_t)H * W <= ((int64_t)1 << 30), "demosaic_fwd: a plane above 2^30 pixels (H=%d W=%d)", H, W);
    DCPT_CHECK_ARG((flags & ~(DCPT_DEMOSAIC_BILINEAR | DCPT_DEMOSAIC_UINT8_IO)) == 0, "demosaic_fwd: unknown flags 0x%x", flags);
    return launch_demosaic_fwd(x, y, B, C, H, W, flags, (hipStream_t)stream);
}

extern "C" int dcpt_inpaint_lines_fwd(const float* x, const int* lines, const int* meta, float* y, int B, int C, int H, int W,
                                      dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && lines && meta && y, "inpaint_lines_fwd: null argument");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0, "inpaint_lines_fwd: bad shape (B=%d C=%d H=%d W=%d)", B, C, H, W);
    DCPT_CHECK_ARG(C == 1 || C == 3, "inpaint_lines_fwd: C must be 1 or 3 (got %d)", C);
    DCPT_CHECK_ARG(H <= 16384 && W <= 16384, "inpaint_lines_fwd: H or W above 16384 (H=%d W=%d)", H, W);
    DCPT_CHECK_ARG(B <= 65535, "inpaint_lines_fwd: B above 65535 (got %d)", B);
    return launch_inpaint_lines_fwd(x, lines, meta, y, B, C, H, W, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Gaussian noise from a per-image Philox stream (noise.hip)
extern "C" int dcpt_gauss_noise_fwd(const float* x, const float* sigma, const long long* key, const int* gray, float* y, int B, int C, int H,
                                    int W, int flags, dcpt_stream_t stream) {
    DCPT_CHECK_ARG((flags & ~(DCPT_NOISE_CLIP | DCPT_NOISE_ROUND8 | DCPT_NOISE_ONLY)) == 0, "gauss_noise_fwd: unknown flags 0x%x", flags);
    DCPT_CHECK_ARG((x || (flags & DCPT_NOISE_ONLY)) && sigma && key && y, "gauss_noise_fwd: null argument");
    DCPT_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "gauss_noise_fwd: bad shape (B=%d C=%d H=%d W=%d)", B, C, H, W);
    // (the counter's first word holds element / 4; compared by division: C * H * W itself may leave 64 bits)
    DCPT_CHECK_ARG((int64_t)C <= (((int64_t)1 << 34) - 1) / ((int64_t)H * W), "gauss_noise_fwd: C * H * W must stay below 2^34 (C=%d H=%d W=%d)",
                   C, H, W);
    DCPT_CHECK_ARG((int64_t)B <= ((int64_t)1 << 40) / ((int64_t)C * H * W), "gauss_noise_fwd: a batch above 2^40 elements (B=%d)", B);
    return launch_gauss_noise_fwd(x, sigma, key, gray, y, B, C, H, W, flags, (hipStream_t)stream);
}

// Poisson (shot) noise on the same stream: a level-count pass and the sampler (noise.hip)
namespace {
const char* poisson_check(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return "bad shape";
    if ((int64_t)C > (((int64_t)1 << 34) - 1) / ((int64_t)H * W)) return "C * H * W must stay below 2^34";
    if ((int64_t)B > ((int64_t)1 << 40) / ((int64_t)C * H * W)) return "a batch above 2^40 elements";
    return nullptr;
}
}  // namespace

extern "C" size_t dcpt_poisson_noise_ws_bytes(int B, int C, int H, int W) {
    return poisson_check(B, C, H, W) ? 0 : poisson_noise_ws_bytes(B, C, H, W);
}

extern "C" int dcpt_poisson_noise_fwd(const float* x, const float* scale, const long long* key, const int* gray, float* y, void* ws,
                                      size_t ws_bytes, int B, int C, int H, int W, int flags, dcpt_stream_t stream) {
    DCPT_CHECK_ARG((flags & ~(DCPT_NOISE_CLIP | DCPT_NOISE_ROUND8 | DCPT_NOISE_ONLY)) == 0, "poisson_noise_fwd: unknown flags 0x%x", flags);
    DCPT_CHECK_ARG(x && scale && key && y && ws, "poisson_noise_fwd: null argument");   // (x also with DCPT_NOISE_ONLY: the rate depends on it)
    const char* bad = poisson_check(B, C, H, W);
    DCPT_CHECK_ARG(!bad, "poisson_noise_fwd: %s (B=%d C=%d H=%d W=%d)", bad, B, C, H, W);
    DCPT_CHECK_ARG(!gray || C == 1 || C == 3, "poisson_noise_fwd: gray noise needs C = 1 or 3 (got %d)", C);
    DCPT_CHECK_WS("poisson_noise_fwd", ws, ws_bytes, dcpt_poisson_noise_ws_bytes(B, C, H, W));
    return launch_poisson_noise_fwd(x, scale, key, gray, y, ws, B, C, H, W, flags, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Synthetic blur: a K x K correlation per image under reflect padding (blur.hip)
extern "C" int dcpt_filter2d_fwd(const float* x, const float* kern, float* y, int B, int C, int H, int W, int K, int kern_per_image,
                                 dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && kern && y, "filter2d_fwd: null argument");
    DCPT_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1, "filter2d_fwd: bad shape (B=%d C=%d H=%d W=%d)", B, C, H, W);
    DCPT_CHECK_ARG(K >= 1 && K <= 51 && (K & 1) == 1, "filter2d_fwd: K must be odd and lie in 1..51 (got %d)", K);
    DCPT_CHECK_ARG(K / 2 < H && K / 2 < W, "filter2d_fwd: the reflect padding K / 2 = %d must be smaller than H and W (H=%d W=%d)", K / 2, H, W);
    const int64_t tiles = cdiv64(W, 64) * cdiv64(H, 32);   // (blur.hip: one workgroup per 32 x 64 tile of a plane, a one-dimensional grid)
    DCPT_CHECK_ARG((int64_t)B * C <= (int64_t)0x7fffffff / tiles, "filter2d_fwd: more than 2^31 - 1 tiles of 32 x 64 (B=%d C=%d H=%d W=%d)", B, C,
                   H, W);
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    const uint64_t bytes = (uint64_t)B * C * H * W * sizeof(float);   // (below 2^31 * 2048 * 4)
    DCPT_CHECK_ARG(xa + bytes <= ya || ya + bytes <= xa, "filter2d_fwd: y overlaps x (a tile reads its neighbours' pixels: not in place)");
    return launch_filter2d_fwd(x, kern, y, B, C, H, W, K, kern_per_image != 0, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// The resize of the second-order degradation chain: F.interpolate's area / bilinear / bicubic (resize.hip)
extern "C" int dcpt_interp_fwd(const float* x, float* y, int B, int C, int H, int W, int Ho, int Wo, int mode, double ratio_h, double ratio_w,
                               int flags, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(x && y, "interp_fwd: null argument");
    DCPT_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "interp_fwd: bad shape (B=%d C=%d H=%d W=%d Ho=%d Wo=%d)", B, C, H,
                   W, Ho, Wo);
    DCPT_CHECK_ARG(mode == DCPT_INTERP_AREA || mode == DCPT_INTERP_BILINEAR || mode == DCPT_INTERP_BICUBIC,
                   "interp_fwd: unknown mode %d (0 area, 1 bilinear, 2 bicubic)", mode);
    DCPT_CHECK_ARG((flags & ~(DCPT_INTERP_CLIP | DCPT_INTERP_ROUND8)) == 0, "interp_fwd: unknown flags 0x%x", flags);
    const int64_t pin = (int64_t)H * W, pout = (int64_t)Ho * Wo, cap = (int64_t)1 << 30;
    DCPT_CHECK_ARG(pin <= cap && pout <= cap, "interp_fwd: a plane above 2^30 pixels (H=%d W=%d Ho=%d Wo=%d)", H, W, Ho, Wo);
    DCPT_CHECK_ARG((int64_t)B * C <= ((int64_t)1 << 40) / (pin > pout ? pin : pout), "interp_fwd: a batch above 2^40 elements (B=%d C=%d)", B, C);
    if (mode != DCPT_INTERP_AREA)   // (the area taps are made from the sizes alone; the comparisons are false for a NaN)
        DCPT_CHECK_ARG(ratio_h > 0.0 && ratio_h <= 0x1p30 && ratio_w > 0.0 && ratio_w <= 0x1p30,
                       "interp_fwd: the ratios must lie in (0, 2^30] (ratio_h=%g ratio_w=%g)", ratio_h, ratio_w);
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    const uint64_t xbytes = (uint64_t)B * C * pin * sizeof(float), ybytes = (uint64_t)B * C * pout * sizeof(float);
    DCPT_CHECK_ARG(xa + xbytes <= ya || ya + ybytes <= xa, "interp_fwd: y overlaps x (an output reads several source pixels: not in place)");
    return launch_interp_fwd(x, y, B, C, H, W, Ho, Wo, mode, ratio_h, ratio_w, flags, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// The kNN degradation probe: fp64 squared distances on the fp64 MFMA, and the neighbour vote (knn.hip)
namespace {
// the effective chunk count of a call, or 0 with `why` set for a refused shape
int pdist2_ksplit(int Nq, int Nt, long long D, int ksplit, const char** why) {
    *why = nullptr;
    if (Nq < 1 || Nt < 1 || D < 1) *why = "Nq, Nt and D must be at least 1";
    else if (Nq > PDIST2_MAX_ROWS || Nt > PDIST2_MAX_ROWS) *why = "more than 65535 rows";
    else if (ksplit < 0 || (long long)ksplit > (D + 3) / 4) *why = "ksplit must lie in 0 .. ceil(D / 4)";
    else if (ksplit > PDIST2_MAX_KSPLIT) *why = "ksplit above 65535";
    if (*why) return 0;
    return ksplit ? ksplit : pdist2_auto_ksplit(Nq, Nt, D);
}
}  // namespace

extern "C" size_t dcpt_pdist2_ws_bytes(int Nq, int Nt, long long D, int ksplit) {
    const char* why;
    const int ks = pdist2_ksplit(Nq, Nt, D, ksplit, &why);
    return ks ? pdist2_ws_bytes(Nq, Nt, ks) : 0;
}

extern "C" int dcpt_pdist2_fwd(const void* xq, const void* xt, double* d2, void* ws, size_t ws_bytes, int Nq, int Nt, long long D, long long ldq,
                               long long ldt, long long ldd, int ksplit, int flags, dcpt_stream_t stream) {
    DCPT_CHECK_ARG((flags & ~DCPT_PDIST_BF16) == 0, "pdist2_fwd: unknown flags 0x%x", flags);
    DCPT_CHECK_ARG(xq && xt && d2 && ws, "pdist2_fwd: null argument");
    const char* why;
    const int ks = pdist2_ksplit(Nq, Nt, D, ksplit, &why);
    DCPT_CHECK_ARG(ks, "pdist2_fwd: %s (Nq=%d Nt=%d D=%lld ksplit=%d)", why, Nq, Nt, D, ksplit);
    DCPT_CHECK_ARG(ldq >= D && ldt >= D && ldd >= Nt, "pdist2_fwd: a leading dimension below its extent (ldq=%lld ldt=%lld D=%lld ldd=%lld Nt=%d)",
                   ldq, ldt, D, ldd, Nt);
    DCPT_CHECK_WS("pdist2_fwd", ws, ws_bytes, pdist2_ws_bytes(Nq, Nt, ks));
    return launch_pdist2_fwd(xq, xt, d2, ws, Nq, Nt, D, ldq, ldt, ldd, ks, (flags & DCPT_PDIST_BF16) != 0, (hipStream_t)stream);
}

extern "C" int dcpt_knn_vote_fwd(const double* d2, long long ldd, const int* q_idx, const int* t_idx, const int* labels, int S, int nq, int nt, int k,
                                 int* nbr, double* nbr_d2, int* pred, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(d2 && q_idx && t_idx && labels && nbr && nbr_d2 && pred, "knn_vote_fwd: null argument");
    DCPT_CHECK_ARG(S >= 1 && nq >= 1 && nt >= 1, "knn_vote_fwd: S, nq and nt must be at least 1 (S=%d nq=%d nt=%d)", S, nq, nt);
    DCPT_CHECK_ARG(k >= 1 && k <= 32 && k <= nt, "knn_vote_fwd: k must lie in 1 .. min(32, nt) (k=%d nt=%d)", k, nt);
    DCPT_CHECK_ARG(ldd >= 1, "knn_vote_fwd: bad leading dimension (ldd=%lld)", ldd);
    DCPT_CHECK_ARG((int64_t)S * nq <= (int64_t)0x7fffffff, "knn_vote_fwd: more than 2^31 - 1 queries over the splits (S=%d nq=%d)", S, nq);
    return launch_knn_vote_fwd(d2, ldd, q_idx, t_idx, labels, S, nq, nt, k, nbr, nbr_d2, pred, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Exact t-SNE on the distance matrix of the probe (tsne.hip)
namespace {
bool tsne_finite(double v) { return v == v && v - v == 0.0; }
}  // namespace

extern "C" size_t dcpt_tsne_steps_ws_bytes(int N) { return (N >= 2 && N <= TSNE_MAX_ROWS) ? tsne_ws_bytes(N) : 0; }

extern "C" int dcpt_tsne_affinity_fwd(const double* d2, long long ldd, double* pcond, long long ldp, double* beta, int* steps, int N,
                                      double perplexity, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(d2 && pcond && beta && steps, "tsne_affinity_fwd: null argument");
    DCPT_CHECK_ARG(N >= 2 && N <= TSNE_MAX_ROWS, "tsne_affinity_fwd: N must lie in 2 .. 65535 (N=%d)", N);
    DCPT_CHECK_ARG(tsne_finite(perplexity) && perplexity >= 1.0 && perplexity < (double)N,
                   "tsne_affinity_fwd: the perplexity must be finite and lie in [1, N) (perplexity=%g N=%d)", perplexity, N);
    DCPT_CHECK_ARG(ldd >= N && ldp >= N, "tsne_affinity_fwd: a leading dimension below N (ldd=%lld ldp=%lld N=%d)", ldd, ldp, N);
    DCPT_CHECK_ARG((const void*)d2 != (const void*)pcond, "tsne_affinity_fwd: pcond must not be d2 (every step reads the distances again)");
    return launch_tsne_affinity_fwd(d2, ldd, pcond, ldp, beta, steps, N, perplexity, (hipStream_t)stream);
}

extern "C" int dcpt_tsne_joint_fwd(const double* pcond, long long ldp, double* P, long long ldo, void* ws, size_t ws_bytes, int N,
                                   dcpt_stream_t stream) {
    DCPT_CHECK_ARG(pcond && P, "tsne_joint_fwd: null argument");
    DCPT_CHECK_ARG(N >= 2 && N <= TSNE_MAX_ROWS, "tsne_joint_fwd: N must lie in 2 .. 65535 (N=%d)", N);
    DCPT_CHECK_ARG(ldp >= N && ldo >= N, "tsne_joint_fwd: a leading dimension below N (ldp=%lld ldo=%lld N=%d)", ldp, ldo, N);
    DCPT_CHECK_ARG((const void*)pcond != (const void*)P || ldp == ldo, "tsne_joint_fwd: P over pcond needs the same leading dimension");
    DCPT_CHECK_WS("tsne_joint_fwd", ws, ws_bytes, tsne_ws_bytes(N));
    return launch_tsne_joint_fwd(pcond, ldp, P, ldo, ws, N, (hipStream_t)stream);
}

extern "C" int dcpt_tsne_steps_fwd(const double* P, long long ldp, double* Y, double* update, double* gains, double* stats, void* ws,
                                   size_t ws_bytes, int N, int out_dims, int n_steps, double exaggeration, double momentum, double lr,
                                   double min_gain, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(P && Y && update && gains && stats, "tsne_steps_fwd: null argument");
    DCPT_CHECK_ARG(out_dims == 2, "tsne_steps_fwd: only two output dimensions exist (out_dims=%d)", out_dims);
    DCPT_CHECK_ARG(N >= 2 && N <= TSNE_MAX_ROWS, "tsne_steps_fwd: N must lie in 2 .. 65535 (N=%d)", N);
    DCPT_CHECK_ARG(ldp >= N, "tsne_steps_fwd: a leading dimension below N (ldp=%lld N=%d)", ldp, N);
    DCPT_CHECK_ARG(n_steps >= 0, "tsne_steps_fwd: n_steps below 0 (%d)", n_steps);
    DCPT_CHECK_ARG(tsne_finite(exaggeration) && tsne_finite(momentum) && tsne_finite(lr) && tsne_finite(min_gain),
                   "tsne_steps_fwd: exaggeration, momentum, lr and min_gain must be finite");
    DCPT_CHECK_ARG(((uintptr_t)Y & 15) == 0, "tsne_steps_fwd: Y must be 16-byte aligned (a point is read as one pair)");
    DCPT_CHECK_WS("tsne_steps_fwd", ws, ws_bytes, tsne_ws_bytes(N));
    return launch_tsne_steps_fwd(P, ldp, Y, update, gains, stats, ws, N, n_steps, exaggeration, momentum, lr, min_gain, (hipStream_t)stream);
}

extern "C" int dcpt_tsne_kl_fwd(const double* P, long long ldp, const double* Y, double* grad, double* stats, void* ws, size_t ws_bytes, int N,
                                int out_dims, double exaggeration, dcpt_stream_t stream) {
    DCPT_CHECK_ARG(P && Y && grad && stats, "tsne_kl_fwd: null argument");
    DCPT_CHECK_ARG(out_dims == 2, "tsne_kl_fwd: only two output dimensions exist (out_dims=%d)", out_dims);
    DCPT_CHECK_ARG(N >= 2 && N <= TSNE_MAX_ROWS, "tsne_kl_fwd: N must lie in 2 .. 65535 (N=%d)", N);
    DCPT_CHECK_ARG(ldp >= N, "tsne_kl_fwd: a leading dimension below N (ldp=%lld N=%d)", ldp, N);
    DCPT_CHECK_ARG(tsne_finite(exaggeration), "tsne_kl_fwd: the exaggeration must be finite");
    DCPT_CHECK_ARG(((uintptr_t)Y & 15) == 0, "tsne_kl_fwd: Y must be 16-byte aligned (a point is read as one pair)");
    DCPT_CHECK_WS("tsne_kl_fwd", ws, ws_bytes, tsne_ws_bytes(N));
    return launch_tsne_kl_fwd(P, ldp, Y, grad, stats, ws, N, exaggeration, (hipStream_t)stream);
}
