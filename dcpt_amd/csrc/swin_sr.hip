// SwinIR super-resolution tail and the "3conv" residual (reference basicsr/archs/swinir_arch.py):
//   conv_before_upsample / conv_hr   y = lrelu(conv3x3(x) + b, slope), Cin -> Cout          dcpt_conv3x3_act_fwd/bwd      (:983-985, :1100)
//   conv_up1 / conv_up2              y = lrelu(conv3x3(nearest2x(x)) + b, slope), C -> C    dcpt_up2_conv3x3_act_fwd/bwd  (:1085-1099)
//   UpsampleOneStep                  img = PixelShuffle(r)(conv3x3(x) + b), C -> r^2 Cimg   dcpt_conv3x3_ps_out_fwd/bwd   (:771-787)
//   RSTB conv / conv_after_body      y = res + conv3x3(lrelu(conv1x1(lrelu(conv3x3(x)))))   dcpt_conv3conv_res_fwd/bwd    (:608-616, :969-977)
//
// Feature maps are NHWC rows [M][C].  Every conv is an implicit GEMM on the fp32 NT kernel (A_CONV3; A_CONV3UP reads the source pixel
// (h' >> 1, w' >> 1) of each tap of the 2H x 2W grid, so the up-sampled map never exists in memory), the LeakyReLU is the GEMM's
// epilogue (E_LRELU).  Backward: the activation's mask comes from the sign of the SAVED OUTPUT (slope >= 0: y > 0 <=> pre-activation
// > 0; y == 0 takes the slope branch, as torch does) -- applied to dy in one bandwidth pass for the single-conv nodes, and in the
// dgrad GEMM's epilogue (E_LRELU with res = the saved map) inside the 3conv chain, the way RCAB applies its ReLU mask; dx from the
// flipped-tap GEMM; dw / db from the TN kernel with its deterministic slab reduce.  No atomics.
// The up-sampled conv's dgrad runs on the 2H x 2W grid and a bandwidth kernel sums each 2 x 2 block.
// The one-step upsampler's GEMM has N = r^2 Cimg = 12 / 27 / 48 columns: the weight / bias rows are zero-padded to a multiple of 4,
// the GEMM writes [M][Npad] rows to the workspace and a bandwidth kernel shuffles them into the NCHW image (conv channel
// c r^2 + i r + j is image channel c at sub-pixel (i, j)).
#include "gemm.h"
#include "kernels.h"
#include "prof.h"
#include "../../include/dcpt_hip.h"

namespace {

constexpr float SLOPE_3CONV = 0.2f;

// dz = dy * (y > 0 ? 1 : slope)
__global__ void lrelu_mask_kernel(const float4* __restrict__ dy, const float4* __restrict__ y, float4* __restrict__ dz, int64_t n4, float slope) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const float4 g = dy[e], v = y[e];
        dz[e] = make_float4(v.x > 0.f ? g.x : slope * g.x, v.y > 0.f ? g.y : slope * g.y, v.z > 0.f ? g.z : slope * g.z,
                            v.w > 0.f ? g.w : slope * g.w);
    }
}

// dx[b][h][w][c] = sum of the 2 x 2 block of du [B][2H][2W][C]  (float4 groups of c)
__global__ void sum2x2_kernel(const float4* __restrict__ du, float4* __restrict__ dx, int64_t n4, int H, int W, int C4) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(e % C4);
        const int64_t m = e / C4;
        const int w = (int)(m % W);
        const int64_t t = m / W;
        const int h = (int)(t % H);
        const int64_t b = t / H;
        const int64_t r0 = ((b * (2 * H) + 2 * h) * (int64_t)(2 * W) + 2 * w) * C4 + c4, r1 = r0 + (int64_t)(2 * W) * C4;
        dx[e] = f4_add(f4_add(du[r0], du[r0 + C4]), f4_add(du[r1], du[r1 + C4]));
    }
}

// out[e] = e < nin ? in[e] : 0   (zero-padded copy; nout == nin: plain copy)
__global__ void pad_copy_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t nin, int64_t nout) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nout; e += (int64_t)gridDim.x * blockDim.x)
        out[e] = e < nin ? in[e] : 0.f;
}

// img[b][c][r h + i][r w + j] = z[m][c r^2 + i r + j]   (one thread per image element: coalesced stores)
__global__ void ps_img_scatter_kernel(const float* __restrict__ z, float* __restrict__ img, int64_t n, int H, int W, int Cimg, int r, int ldz) {
    const int rH = r * H, rW = r * W;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int wf = (int)(e % rW);
        int64_t t = e / rW;
        const int hf = (int)(t % rH);
        t /= rH;
        const int c = (int)(t % Cimg);
        const int64_t b = t / Cimg;
        const int64_t m = (b * H + hf / r) * W + wf / r;
        img[e] = z[m * ldz + c * r * r + (hf % r) * r + wf % r];
    }
}

// dz[m][c r^2 + i r + j] = dimg[b][c][r h + i][r w + j], padding columns (>= N) = 0   (one thread per dz element)
__global__ void ps_img_gather_kernel(const float* __restrict__ dimg, float* __restrict__ dz, int64_t n, int H, int W, int Cimg, int r, int ldz) {
    const int rH = r * H, rW = r * W, N = r * r * Cimg;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(e % ldz);
        const int64_t m = e / ldz;
        float v = 0.f;
        if (col < N) {
            const int c = col / (r * r), ij = col % (r * r);
            const int w = (int)(m % W);
            const int64_t t = m / W;
            const int h = (int)(t % H);
            const int64_t b = t / H;
            v = dimg[((b * Cimg + c) * rH + r * h + ij / r) * (int64_t)rW + r * w + ij % r];
        }
        dz[e] = v;
    }
}

int lrelu_mask(const float* dy, const float* y, float* dz, int64_t n, float slope, hipStream_t s) {
    lrelu_mask_kernel<<<dim3(ew_grid(n / 4)), dim3(256), 0, s>>>(reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(y),
                                                                 reinterpret_cast<float4*>(dz), n / 4, slope);
    DCPT_CHECK_LAUNCH("lrelu_mask");
    return DCPT_OK;
}

bool map_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1 << 28) && (int64_t)B * H * W < (1ll << 40); }
bool slope_ok(float slope) { return slope >= 0.f && slope <= 1.f; }

// ---- conv + LeakyReLU (optionally over the nearest-2x up-sampling) ------------------------------------------------
struct ActWs {
    float* wp;            // packed weights: forward [Cout][9 Cin], backward [Cin][9 Cout]
    float *dz, *du;       // backward: masked dy [Mo][Cout]; up2: dgrad on the 2H x 2W grid [Mo][Cin]
    float *slab, *colsum;
};
// up = 1: output grid 2H x 2W (Mo = 4 M)
size_t act_layout(int B, int H, int W, int Cin, int Cout, int up, int backward, void* base, size_t bytes, ActWs* out) {
    WsAlloc a(base, bytes);
    ActWs w{};
    const int64_t Mo = (int64_t)B * H * W * (up ? 4 : 1);
    w.wp = a.get<float>((size_t)9 * Cin * Cout);
    if (backward) {
        w.dz = a.get<float>((size_t)Mo * Cout);
        if (up) w.du = a.get<float>((size_t)Mo * Cin);
        size_t sl = 0, cs = 0;
        wgrad_need(Mo, Cout, 9 * Cin, &sl, &cs);
        w.slab = a.get<float>(sl);
        w.colsum = a.get<float>(cs);
    }
    if (out) *out = w;
    return a.off;
}
bool act_dims_ok(int B, int H, int W, int Cin, int Cout, int up) {
    return map_ok(B, H, W) && Cin > 0 && Cout > 0 && Cin % 4 == 0 && Cout % 4 == 0 && Cin <= 4096 && Cout <= 4096 && (!up || Cin == Cout);
}

int act_fwd(const char* who, const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H, int W, int Cin,
            int Cout, int up, float slope, hipStream_t s) {
    DCPT_CHECK_ARG(x && w && bias && y, "%s: null argument", who);
    DCPT_CHECK_ARG(act_dims_ok(B, H, W, Cin, Cout, up) && slope_ok(slope),
                   "%s: B=%d H=%d W=%d Cin=%d Cout=%d slope=%g (channels positive multiples of 4, 0 <= slope <= 1)", who, B, H, W, Cin, Cout,
                   (double)slope);
    ActWs aw;
    const size_t need = act_layout(B, H, W, Cin, Cout, up, 0, ws, ws_bytes, &aw);
    DCPT_CHECK_WS(who, ws, ws_bytes, need);
    trace_tag(up ? "swinsr_up2_conv_act_fwd" : "swinsr_conv_act_fwd");
    DCPT_TRY(launch_wpack(w, aw.wp, nullptr, Cout, 9 * Cin, WP_CONV3, s));
    GemmNT g = gemm_nt_conv3(x, B, H, W, Cin, aw.wp, Cout, y, Cout);
    if (up) g.M *= 4;   // the rows are the pixels of the 2H x 2W grid
    g.bias = bias; g.slope = slope;
    return launch_gemm_nt(g, up ? A_CONV3UP : A_CONV3, E_LRELU, s);
}

int act_bwd(const char* who, const float* dy, const float* x, const float* y, const float* w, float* dx, float* dw, float* dbias, void* ws,
            size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int up, float slope, hipStream_t s) {
    DCPT_CHECK_ARG(dy && x && y && w && dx && dw && dbias, "%s: null argument", who);
    DCPT_CHECK_ARG(act_dims_ok(B, H, W, Cin, Cout, up) && slope_ok(slope),
                   "%s: B=%d H=%d W=%d Cin=%d Cout=%d slope=%g (channels positive multiples of 4, 0 <= slope <= 1)", who, B, H, W, Cin, Cout,
                   (double)slope);
    ActWs aw;
    const size_t need = act_layout(B, H, W, Cin, Cout, up, 1, ws, ws_bytes, &aw);
    DCPT_CHECK_WS(who, ws, ws_bytes, need);
    trace_tag(up ? "swinsr_up2_conv_act_bwd" : "swinsr_conv_act_bwd");
    const int64_t M = (int64_t)B * H * W, Mo = up ? 4 * M : M;
    DCPT_TRY(lrelu_mask(dy, y, aw.dz, Mo * Cout, slope, s));
    if (!up) return launch_conv3_bwd(aw.dz, x, w, aw.wp, B, H, W, Cin, Cout, E_PLAIN, nullptr, 0.f, dx, aw.slab, aw.colsum, dw, dbias, s);
    // dgrad on the 2H x 2W output grid: a 3x3 conv of dz with the transposed, flipped weights, then the sum of each 2 x 2 block
    DCPT_TRY(launch_wpack(w, aw.wp, nullptr, Cout, 9 * Cin, WP_CONV3_T, s));
    DCPT_TRY(launch_gemm_nt(gemm_nt_conv3(aw.dz, B, 2 * H, 2 * W, Cout, aw.wp, Cin, aw.du, Cin), A_CONV3, E_PLAIN, s));
    const int64_t n4 = M * Cin / 4;
    sum2x2_kernel<<<dim3(ew_grid(n4)), dim3(256), 0, s>>>(reinterpret_cast<const float4*>(aw.du), reinterpret_cast<float4*>(dx), n4, H, W,
                                                          Cin / 4);
    DCPT_CHECK_LAUNCH("sum2x2");
    GemmTN t{};
    t.gH = H; t.gW = W; t.gC = Cin;   // the coarse map x; the rows are on the fine grid
    return launch_wgrad(t, A_CONV3UP, aw.dz, Cout, Cout, x, Cin, 9 * Cin, Mo, aw.slab, aw.colsum, dw, dbias, WR_CONV3, s);
}

// ---- one-step upsampler -------------------------------------------------------------------------------------
struct PsOutWs {
    float *wq, *bq;    // weight / bias rows zero-padded to Npad
    float *wp;         // packed weights: forward [Npad][9C], backward [C][9 Npad]
    float *z;          // forward: conv output rows [M][Npad]; backward: gathered dy
    float *dwq, *dbq;
    float *slab, *colsum;
};
inline int ps_npad(int Cimg, int r) { return (r * r * Cimg + 3) & ~3; }

size_t psout_layout(int B, int H, int W, int C, int Cimg, int r, int backward, void* base, size_t bytes, PsOutWs* out) {
    WsAlloc a(base, bytes);
    PsOutWs w{};
    const int64_t M = (int64_t)B * H * W;
    const int Np = ps_npad(Cimg, r);
    w.wq = a.get<float>((size_t)9 * Np * C);
    w.wp = a.get<float>((size_t)9 * Np * C);
    w.bq = a.get<float>((size_t)Np);
    w.z = a.get<float>((size_t)M * Np);
    if (backward) {
        w.dwq = a.get<float>((size_t)9 * Np * C);
        w.dbq = a.get<float>((size_t)Np);
        size_t sl = 0, cs = 0;
        wgrad_need(M, Np, 9 * C, &sl, &cs);
        w.slab = a.get<float>(sl);
        w.colsum = a.get<float>(cs);
    }
    if (out) *out = w;
    return a.off;
}
bool psout_dims_ok(int B, int H, int W, int C, int Cimg, int r) {
    return map_ok(B, H, W) && C > 0 && C % 4 == 0 && C <= 4096 && Cimg >= 1 && Cimg <= 4 && r >= 2 && r <= 4 &&
           (double)r * H * r * W < (double)(1 << 30);
}
int check_psout(int B, int H, int W, int C, int Cimg, int r, const char* who) {
    DCPT_CHECK_ARG(psout_dims_ok(B, H, W, C, Cimg, r), "%s: B=%d H=%d W=%d C=%d Cimg=%d r=%d (C a positive multiple of 4, Cimg 1..4, r 2..4)", who,
                   B, H, W, C, Cimg, r);
    return DCPT_OK;
}

// ---- 3conv residual ----------------------------------------------------------------------------------------------
struct C3Ws {
    float *wp1, *wp3;     // forward: packed [Cq][9C], [C][9Cq]; backward: wp1 holds whichever transposed pack is in use
    float *wT2;           // backward: [Cq][Cq] transposed 1x1 weight
    float *a1, *a2;       // forward intermediates when the caller keeps nothing
    float *d1, *d2;       // backward: gradients of the two activated maps [M][Cq]
    float *slab, *colsum;
};
size_t c3_layout(int B, int H, int W, int C, int backward, void* base, size_t bytes, C3Ws* out) {
    WsAlloc a(base, bytes);
    C3Ws w{};
    const int64_t M = (int64_t)B * H * W;
    const int Cq = C / 4;
    w.wp1 = a.get<float>((size_t)9 * C * Cq);
    if (!backward) {
        w.wp3 = a.get<float>((size_t)9 * C * Cq);
        w.a1 = a.get<float>((size_t)M * Cq);
        w.a2 = a.get<float>((size_t)M * Cq);
    } else {
        w.wT2 = a.get<float>((size_t)Cq * Cq);
        w.d1 = a.get<float>((size_t)M * Cq);
        w.d2 = a.get<float>((size_t)M * Cq);
        size_t sl = 0, cs = 0;
        wgrad_need(M, C, 9 * Cq, &sl, &cs);
        wgrad_need(M, Cq, Cq, &sl, &cs);
        wgrad_need(M, Cq, 9 * C, &sl, &cs);
        w.slab = a.get<float>(sl);
        w.colsum = a.get<float>(cs);
    }
    if (out) *out = w;
    return a.off;
}
bool c3_dims_ok(int B, int H, int W, int C) { return map_ok(B, H, W) && C > 0 && C % 16 == 0 && C <= 4096; }
int check_c3(int B, int H, int W, int C, const char* who) {
    DCPT_CHECK_ARG(c3_dims_ok(B, H, W, C), "%s: B=%d H=%d W=%d C=%d (C a positive multiple of 16: the inner maps are C / 4 wide, in float4 groups)",
                   who, B, H, W, C);
    return DCPT_OK;
}

}  // namespace

// =====================================================================================================
extern "C" size_t dcpt_conv3x3_act_ws_bytes(int B, int H, int W, int Cin, int Cout, int backward) {
    if (!act_dims_ok(B, H, W, Cin, Cout, 0)) return 0;
    return act_layout(B, H, W, Cin, Cout, 0, backward, nullptr, 0, nullptr);
}
extern "C" int dcpt_conv3x3_act_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H, int W,
                                    int Cin, int Cout, float slope, dcpt_stream_t stream) {
    return act_fwd("conv3x3_act_fwd", x, w, bias, y, ws, ws_bytes, B, H, W, Cin, Cout, 0, slope, (hipStream_t)stream);
}
extern "C" int dcpt_conv3x3_act_bwd(const float* dy, const float* x, const float* y, const float* w, float* dx, float* dw, float* dbias, void* ws,
                                    size_t ws_bytes, int B, int H, int W, int Cin, int Cout, float slope, dcpt_stream_t stream) {
    return act_bwd("conv3x3_act_bwd", dy, x, y, w, dx, dw, dbias, ws, ws_bytes, B, H, W, Cin, Cout, 0, slope, (hipStream_t)stream);
}

extern "C" size_t dcpt_up2_conv3x3_act_ws_bytes(int B, int H, int W, int C, int backward) {
    if (!act_dims_ok(B, H, W, C, C, 1)) return 0;
    return act_layout(B, H, W, C, C, 1, backward, nullptr, 0, nullptr);
}
extern "C" int dcpt_up2_conv3x3_act_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H,
                                        int W, int C, float slope, dcpt_stream_t stream) {
    return act_fwd("up2_conv3x3_act_fwd", x, w, bias, y, ws, ws_bytes, B, H, W, C, C, 1, slope, (hipStream_t)stream);
}
extern "C" int dcpt_up2_conv3x3_act_bwd(const float* dy, const float* x, const float* y, const float* w, float* dx, float* dw, float* dbias,
                                        void* ws, size_t ws_bytes, int B, int H, int W, int C, float slope, dcpt_stream_t stream) {
    return act_bwd("up2_conv3x3_act_bwd", dy, x, y, w, dx, dw, dbias, ws, ws_bytes, B, H, W, C, C, 1, slope, (hipStream_t)stream);
}

// =====================================================================================================
extern "C" size_t dcpt_conv3x3_ps_out_ws_bytes(int B, int H, int W, int C, int Cimg, int r, int backward) {
    if (!psout_dims_ok(B, H, W, C, Cimg, r)) return 0;
    return psout_layout(B, H, W, C, Cimg, r, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_conv3x3_ps_out_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H,
                                       int W, int C, int Cimg, int r, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(x && w && bias && y, "conv3x3_ps_out_fwd: null argument");
    DCPT_TRY(check_psout(B, H, W, C, Cimg, r, "conv3x3_ps_out_fwd"));
    PsOutWs pw;
    const size_t need = psout_layout(B, H, W, C, Cimg, r, 0, ws, ws_bytes, &pw);
    DCPT_CHECK_WS("conv3x3_ps_out_fwd", ws, ws_bytes, need);
    const int N = r * r * Cimg, Np = ps_npad(Cimg, r);
    const int64_t M = (int64_t)B * H * W;
    trace_tag("swinsr_ps_out_fwd");
    pad_copy_kernel<<<dim3(ew_grid((int64_t)Np * 9 * C)), dim3(256), 0, s>>>(w, pw.wq, (int64_t)N * 9 * C, (int64_t)Np * 9 * C);
    DCPT_CHECK_LAUNCH("pad_copy");
    pad_copy_kernel<<<dim3(1), dim3(256), 0, s>>>(bias, pw.bq, N, Np);
    DCPT_CHECK_LAUNCH("pad_copy");
    DCPT_TRY(launch_wpack(pw.wq, pw.wp, nullptr, Np, 9 * C, WP_CONV3, s));
    GemmNT g = gemm_nt_conv3(x, B, H, W, C, pw.wp, Np, pw.z, Np);
    g.bias = pw.bq; g.slope = 1.f;
    DCPT_TRY(launch_gemm_nt(g, A_CONV3, E_LRELU, s));   // slope 1: the plain biased conv
    const int64_t n = M * N;
    ps_img_scatter_kernel<<<dim3(ew_grid(n)), dim3(256), 0, s>>>(pw.z, y, n, H, W, Cimg, r, Np);
    DCPT_CHECK_LAUNCH("ps_img_scatter");
    return DCPT_OK;
}

extern "C" int dcpt_conv3x3_ps_out_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, void* ws,
                                       size_t ws_bytes, int B, int H, int W, int C, int Cimg, int r, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(dy && x && w && dx && dw && dbias, "conv3x3_ps_out_bwd: null argument");
    DCPT_TRY(check_psout(B, H, W, C, Cimg, r, "conv3x3_ps_out_bwd"));
    PsOutWs pw;
    const size_t need = psout_layout(B, H, W, C, Cimg, r, 1, ws, ws_bytes, &pw);
    DCPT_CHECK_WS("conv3x3_ps_out_bwd", ws, ws_bytes, need);
    const int N = r * r * Cimg, Np = ps_npad(Cimg, r);
    const int64_t M = (int64_t)B * H * W;
    trace_tag("swinsr_ps_out_bwd");
    ps_img_gather_kernel<<<dim3(ew_grid(M * Np)), dim3(256), 0, s>>>(dy, pw.z, M * Np, H, W, Cimg, r, Np);
    DCPT_CHECK_LAUNCH("ps_img_gather");
    pad_copy_kernel<<<dim3(ew_grid((int64_t)Np * 9 * C)), dim3(256), 0, s>>>(w, pw.wq, (int64_t)N * 9 * C, (int64_t)Np * 9 * C);
    DCPT_CHECK_LAUNCH("pad_copy");
    // dx = conv^T(dz): a 3x3 conv of the Npad-channel map dz with the transposed, flipped weights (the padding rows are zero)
    DCPT_TRY(launch_conv3_bwd(pw.z, x, pw.wq, pw.wp, B, H, W, C, Np, E_PLAIN, nullptr, 0.f, dx, pw.slab, pw.colsum, pw.dwq, pw.dbq, s));
    pad_copy_kernel<<<dim3(ew_grid((int64_t)N * 9 * C)), dim3(256), 0, s>>>(pw.dwq, dw, (int64_t)N * 9 * C, (int64_t)N * 9 * C);
    DCPT_CHECK_LAUNCH("pad_copy");
    pad_copy_kernel<<<dim3(1), dim3(256), 0, s>>>(pw.dbq, dbias, N, N);
    DCPT_CHECK_LAUNCH("pad_copy");
    return DCPT_OK;
}

// =====================================================================================================
extern "C" size_t dcpt_conv3conv_res_ws_bytes(int B, int H, int W, int C, int backward) {
    if (!c3_dims_ok(B, H, W, C)) return 0;
    return c3_layout(B, H, W, C, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_conv3conv_res_fwd(const dcpt_conv3conv_params* p, const float* x, const float* res, float* y, float* a1, float* a2, void* ws,
                                      size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && x && res && y && p->conv1_w && p->conv1_b && p->conv2_w && p->conv2_b && p->conv3_w && p->conv3_b,
                   "conv3conv_res_fwd: null argument");
    DCPT_CHECK_ARG((a1 == nullptr) == (a2 == nullptr), "conv3conv_res_fwd: pass both saved maps or neither");
    DCPT_TRY(check_c3(B, H, W, C, "conv3conv_res_fwd"));
    C3Ws cw;
    const size_t need = c3_layout(B, H, W, C, 0, ws, ws_bytes, &cw);
    DCPT_CHECK_WS("conv3conv_res_fwd", ws, ws_bytes, need);
    const int Cq = C / 4;
    const int64_t M = (int64_t)B * H * W;
    if (!a1) {
        a1 = cw.a1;
        a2 = cw.a2;
    }
    trace_tag("swinsr_conv3conv_fwd");
    DCPT_TRY(launch_wpack(p->conv1_w, cw.wp1, nullptr, Cq, 9 * C, WP_CONV3, s));
    DCPT_TRY(launch_wpack(p->conv3_w, cw.wp3, nullptr, C, 9 * Cq, WP_CONV3, s));
    GemmNT g = gemm_nt_conv3(x, B, H, W, C, cw.wp1, Cq, a1, Cq);
    g.bias = p->conv1_b; g.slope = SLOPE_3CONV;
    DCPT_TRY(launch_gemm_nt(g, A_CONV3, E_LRELU, s));
    g = gemm_nt_linear(a1, Cq, M, Cq, p->conv2_w, Cq, a2, Cq);
    g.bias = p->conv2_b; g.slope = SLOPE_3CONV;
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_LRELU, s));
    g = gemm_nt_conv3(a2, B, H, W, Cq, cw.wp3, C, y, C);
    g.bias = p->conv3_b; g.res = res;
    return launch_gemm_nt(g, A_CONV3, E_RESID, s);
}

extern "C" int dcpt_conv3conv_res_bwd(const dcpt_conv3conv_params* p, const dcpt_conv3conv_params_grads* gr, const float* x, const float* a1,
                                      const float* a2, const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                                      dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && gr && x && a1 && a2 && dy && dx && p->conv1_w && p->conv2_w && p->conv3_w, "conv3conv_res_bwd: null argument");
    DCPT_CHECK_ARG(gr->conv1_w && gr->conv1_b && gr->conv2_w && gr->conv2_b && gr->conv3_w && gr->conv3_b, "conv3conv_res_bwd: null gradient");
    DCPT_TRY(check_c3(B, H, W, C, "conv3conv_res_bwd"));
    C3Ws cw;
    const size_t need = c3_layout(B, H, W, C, 1, ws, ws_bytes, &cw);
    DCPT_CHECK_WS("conv3conv_res_bwd", ws, ws_bytes, need);
    const int Cq = C / 4;
    const int64_t M = (int64_t)B * H * W;
    trace_tag("swinsr_conv3conv_bwd");
    // conv3: d2 = lrelu'(a2) conv3^T(dy);  dW3, db3 from dy and a2
    DCPT_TRY(launch_conv3_bwd(dy, a2, p->conv3_w, cw.wp1, B, H, W, Cq, C, E_LRELU, a2, SLOPE_3CONV, cw.d2, cw.slab, cw.colsum, gr->conv3_w,
                              gr->conv3_b, s));
    // conv2 (1x1): d1 = lrelu'(a1) (d2 W2);  dW2 = d2^T a1, db2 = colsum(d2)
    DCPT_TRY(launch_wpack(p->conv2_w, cw.wT2, nullptr, Cq, Cq, WP_TRANSPOSE, s));
    GemmNT g = gemm_nt_linear(cw.d2, Cq, M, Cq, cw.wT2, Cq, cw.d1, Cq);
    g.res = a1; g.slope = SLOPE_3CONV;
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_LRELU, s));
    DCPT_TRY(launch_wgrad(GemmTN{}, A_PLAIN, cw.d2, Cq, Cq, a1, Cq, Cq, M, cw.slab, cw.colsum, gr->conv2_w, gr->conv2_b, WR_PLAIN, s));
    // conv1: dx = conv1^T(d1);  dW1, db1 from d1 and x   (the residual's gradient is dy itself)
    return launch_conv3_bwd(cw.d1, x, p->conv1_w, cw.wp1, B, H, W, C, Cq, E_PLAIN, nullptr, 0.f, dx, cw.slab, cw.colsum, gr->conv1_w,
                            gr->conv1_b, s);
}
