// RCAN (reference basicsr/archs/rcan_arch.py):
//   RCAB           y = x + res_scale * CA(conv2(relu(conv1(x))))        dcpt_rcab_fwd/bwd
//   CA             t * sigmoid(W2 relu(W1 mean_hw(t) + b1) + b2)         (inside the RCAB calls)
//   Upsample stage y = PixelShuffle(r)(conv3x3(x) + bias), r in {2, 3}   dcpt_conv3x3_ps_fwd/bwd
//
// Feature maps are NHWC rows [M][C] (M = B*H*W).  Both 3x3 convs of an RCAB are implicit GEMMs (A_CONV3) on the fp32 NT kernel:
// conv1 with the bias + ReLU epilogue (E_RELU), conv2 with the bias epilogue that also leaves per-image column sums of its output
// (E_BIASCOL), so the channel-attention pooling needs no second pass over t.  The CA kernel (one workgroup per image) turns those
// sums into the mean and runs the two tiny FCs and the sigmoid; a bandwidth kernel writes y = x + res_scale * t * s[b][c].
// Backward: ds = res_scale * sum_hw dy t (per-image split partials), the CA backward per image (parameter-gradient partials per
// image, reduced over the batch in a fixed order), dt = res_scale dy s + dpooled / HW, conv2 dgrad with the ReLU mask in its
// epilogue (E_RELU with res = h), conv1 dgrad with dx = dy + conv1^T(dh) in a residual epilogue, both weight gradients on the TN
// kernel.  No atomics anywhere: results are bit-identical run to run.
//
// Upsample stage: conv channel c r^2 + i r + j is PixelShuffle's channel c at sub-pixel (i, j).  The weight rows are reordered to
// GEMM column (i r + j) C + c, so that a float4 group of GEMM columns is 4 consecutive channels of one fine pixel, and the GEMM's
// scatter epilogue (E_PSHUF) writes the shuffled image directly.  Backward gathers dy into that column order (one bandwidth pass),
// then runs the dgrad / wgrad GEMMs and puts the weight / bias gradient rows back in the reference's order.
#include "gemm.h"
#include "kernels.h"
#include "prof.h"
#include "../../include/dcpt_hip.h"

namespace {

// ---- channel attention ------------------------------------------------------------------------------
// one workgroup per image b: pooled = (sum of the tile / image column sums) / P, h = relu(W1 pooled + b1), s = sigmoid(W2 h + b2).
// G groups of C threads split the image's tiles (a 256^2 image has 512 of them), then add their G partials in a fixed order.
__global__ __launch_bounds__(256) void ca_fwd_kernel(const float* __restrict__ colpart, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, float* __restrict__ pooled, float* __restrict__ s,
                                                     int P, int C, int Cr, int G) {
    extern __shared__ float sm[];
    float* pm = sm;             // [C]
    float* hz = sm + C;         // [Cr]
    float* gp = hz + Cr;        // [G][C]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t0 = (int64_t)b * P / 128, t1 = ((int64_t)(b + 1) * P - 1) / 128;
    const float invP = 1.f / (float)P;
    for (int e = tid; e < G * C; e += 256) {
        const int c = e % C, g = e / C;
        float acc = 0.f;
#pragma unroll 4
        for (int64_t t = t0 + g; t <= t1; t += G) acc += colpart[(t + b) * C + c];
        gp[e] = acc;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float acc = 0.f;
        for (int g = 0; g < G; ++g) acc += gp[g * C + c];
        pm[c] = acc * invP;
        pooled[(int64_t)b * C + c] = acc * invP;
    }
    __syncthreads();
    for (int j = wave; j < Cr; j += 4) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc += w1[(int64_t)j * C + c] * pm[c];
        acc = wave_sum(acc);
        if (lane == 0) hz[j] = fmaxf(acc + b1[j], 0.f);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float a = b2[c];
        for (int j = 0; j < Cr; ++j) a += w2[(int64_t)c * Cr + j] * hz[j];
        s[(int64_t)b * C + c] = 1.f / (1.f + expf(-a));
    }
}

// y = x + rs * t * s[b][c]   (float4 groups; C % 4 == 0)
__global__ void rcab_scale_kernel(const float4* __restrict__ x, const float4* __restrict__ t, const float* __restrict__ s,
                                  float4* __restrict__ y, int64_t n4, int C, int64_t PC, float rs) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t el = 4 * e;
        const float4 sv = *reinterpret_cast<const float4*>(s + (el / PC) * C + el % C);
        const float4 xv = x[e], tv = t[e];
        y[e] = make_float4(fmaf(rs * tv.x, sv.x, xv.x), fmaf(rs * tv.y, sv.y, xv.y), fmaf(rs * tv.z, sv.z, xv.z), fmaf(rs * tv.w, sv.w, xv.w));
    }
}

// dt = rs * dy * s[b][c] + dpool[b][c]   (dpool already divided by P)
__global__ void rcab_dt_kernel(const float4* __restrict__ dy, const float* __restrict__ s, const float* __restrict__ dpool,
                               float4* __restrict__ dt, int64_t n4, int C, int64_t PC, float rs) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t el = 4 * e;
        const int64_t bc = (el / PC) * C + el % C;
        const float4 sv = *reinterpret_cast<const float4*>(s + bc);
        const float4 dp = *reinterpret_cast<const float4*>(dpool + bc);
        const float4 g = dy[e];
        dt[e] = make_float4(fmaf(rs * g.x, sv.x, dp.x), fmaf(rs * g.y, sv.y, dp.y), fmaf(rs * g.z, sv.z, dp.z), fmaf(rs * g.w, sv.w, dp.w));
    }
}

// part[b][j][c] = sum over rows [j*rps, min((j+1)*rps, P)) of image b of dy * t  (grid (NS, B)); G row subgroups of C columns,
// then a fixed-order sum over the subgroups through LDS
__global__ __launch_bounds__(256) void rcab_dot_kernel(const float* __restrict__ dy, const float* __restrict__ t, float* __restrict__ part,
                                                       int P, int C, int NS, int rps, int G) {
    extern __shared__ float sm[];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lo = j * rps, hi = min((j + 1) * rps, P);
    const int64_t base = (int64_t)b * P * C;
    for (int e = tid; e < G * C; e += 256) {
        const int c = e % C, g = e / C;
        float acc = 0.f;
        for (int r = lo + g; r < hi; r += G) {
            const int64_t o = base + (int64_t)r * C + c;
            acc = fmaf(dy[o], t[o], acc);
        }
        sm[e] = acc;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float acc = 0.f;
        for (int g = 0; g < G; ++g) acc += sm[g * C + c];
        part[((int64_t)b * NS + j) * C + c] = acc;
    }
}

// CA backward of image b (grid B): ds = rs sum_j part, da = ds s (1 - s), z = W1 pooled + b1, dz = [z > 0] W2^T da,
// dpool = (W1^T dz) / P; parameter-gradient partials of this image gp[b] = [dW1 (Cr x C) | db1 (Cr) | dW2 (C x Cr) | db2 (C)]
__global__ __launch_bounds__(256) void ca_bwd_kernel(const float* __restrict__ part, int NS, const float* __restrict__ pooled,
                                                     const float* __restrict__ s, const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, float rs, float* __restrict__ dpool, float* __restrict__ gp,
                                                     int P, int C, int Cr) {
    extern __shared__ float sm[];
    float* pm = sm;             // [C]
    float* da = sm + C;         // [C]
    float* z = sm + 2 * C;      // [Cr]
    float* dz = z + Cr;         // [Cr]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t G = 2 * (int64_t)C * Cr + Cr + C;
    float* g = gp + b * G;
    for (int c = tid; c < C; c += 256) {
        float acc = 0.f;
        for (int j = 0; j < NS; ++j) acc += part[((int64_t)b * NS + j) * C + c];
        const float sv = s[(int64_t)b * C + c];
        da[c] = rs * acc * sv * (1.f - sv);
        pm[c] = pooled[(int64_t)b * C + c];
    }
    __syncthreads();
    for (int j = wave; j < Cr; j += 4) {
        float a = 0.f, d = 0.f;
        for (int c = lane; c < C; c += 64) {
            a += w1[(int64_t)j * C + c] * pm[c];
            d += w2[(int64_t)c * Cr + j] * da[c];
        }
        a = wave_sum(a);
        d = wave_sum(d);
        if (lane == 0) {
            z[j] = a + b1[j];
            dz[j] = a + b1[j] > 0.f ? d : 0.f;
        }
    }
    __syncthreads();
    const float invP = 1.f / (float)P;
    for (int c = tid; c < C; c += 256) {
        float a = 0.f;
        for (int j = 0; j < Cr; ++j) a += w1[(int64_t)j * C + c] * dz[j];
        dpool[(int64_t)b * C + c] = a * invP;
        g[2 * (int64_t)C * Cr + Cr + c] = da[c];
    }
    for (int e = tid; e < C * Cr; e += 256) {
        g[e] = dz[e / C] * pm[e % C];
        g[(int64_t)C * Cr + Cr + e] = da[e / Cr] * fmaxf(z[e % Cr], 0.f);
    }
    for (int j = tid; j < Cr; j += 256) g[(int64_t)C * Cr + j] = dz[j];
}

// sum the per-image partials over the batch (fixed order) into dW1, db1, dW2, db2
__global__ void ca_grad_reduce_kernel(const float* __restrict__ gp, int B, int C, int Cr, float* __restrict__ dw1, float* __restrict__ db1,
                                      float* __restrict__ dw2, float* __restrict__ db2) {
    const int64_t G = 2 * (int64_t)C * Cr + Cr + C;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < G; e += (int64_t)gridDim.x * blockDim.x) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += gp[b * G + e];
        const int64_t CCr = (int64_t)C * Cr;
        if (e < CCr) dw1[e] = acc;
        else if (e < CCr + Cr) db1[e - CCr] = acc;
        else if (e < 2 * CCr + Cr) dw2[e - CCr - Cr] = acc;
        else db2[e - 2 * CCr - Cr] = acc;
    }
}

// ---- pixel shuffle helpers ----------------------------------------------------------------------------
// GEMM column n' = (i r + j) C + c  <->  conv channel c r^2 + i r + j.  dir 0: out[n'] = in[ch(n')]; dir 1: out[ch(n')] = in[n']
// (rows of L floats: the weight's C*9, the bias's 1)
__global__ void ps_rowperm_kernel(const float* __restrict__ in, float* __restrict__ out, int N, int L, int C, int r, int dir) {
    const int64_t n = (int64_t)N * L;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int np = (int)(e / L), k = (int)(e % L);
        const int ch = (np % C) * r * r + np / C;
        if (dir == 0) out[e] = in[(int64_t)ch * L + k];
        else out[(int64_t)ch * L + k] = in[e];
    }
}

// dz[m][(i r + j) C + c] = dy[b][r h + i][r w + j][c]   (float4 groups of c)
__global__ void ps_gather_kernel(const float4* __restrict__ dy, float4* __restrict__ dz, int64_t n4, int H, int W, int C, int r) {
    const int C4 = C / 4, N4 = r * r * C4;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = e / N4;
        const int col = (int)(e % N4);
        const int ij = col / C4, c4 = col % C4;
        const int i = ij / r, j = ij % r;
        const int w = (int)(m % W);
        const int64_t t = m / W;
        const int h = (int)(t % H);
        const int64_t b = t / H;
        dz[e] = dy[((b * (r * H) + r * h + i) * (int64_t)(r * W) + r * w + j) * C4 + c4];
    }
}

// ---- RCAB workspace ---------------------------------------------------------------------------------
int dot_splits(int B, int P) {
    int ns = cdiv(512, B);
    const int maxs = cdiv(P, 64);
    if (ns > maxs) ns = maxs;
    return ns < 1 ? 1 : ns;
}
int dot_groups(int C) { return C >= 256 ? 1 : 256 / C; }

struct RcabWs {
    float *wp1, *wp2;                     // packed weights [C][9C] (backward: transposed for the dgrads)
    float *colpart;                       // forward: [(tiles_m + B - 1)][C] tile / image column sums of t
    float *h, *t, *pooled, *s;            // forward intermediates when the caller keeps nothing
    float *dt, *dh, *dpart, *dpool, *gp;  // backward
    float *slab, *colsum;
    int ns;
};

size_t rcab_layout(int B, int H, int W, int C, int Cr, int backward, void* base, size_t bytes, RcabWs* out) {
    WsAlloc a(base, bytes);
    RcabWs w{};
    const int64_t M = (int64_t)B * H * W;
    w.wp1 = a.get<float>((size_t)9 * C * C);
    w.wp2 = a.get<float>((size_t)9 * C * C);
    if (!backward) {
        w.colpart = a.get<float>((size_t)(cdiv64(M, 128) + B - 1) * C);
        w.h = a.get<float>((size_t)M * C);
        w.t = a.get<float>((size_t)M * C);
        w.pooled = a.get<float>((size_t)B * C);
        w.s = a.get<float>((size_t)B * C);
    } else {
        w.ns = dot_splits(B, H * W);
        w.dt = a.get<float>((size_t)M * C);
        w.dh = a.get<float>((size_t)M * C);
        w.dpart = a.get<float>((size_t)B * w.ns * C);
        w.dpool = a.get<float>((size_t)B * C);
        w.gp = a.get<float>((size_t)B * (2 * (size_t)C * Cr + Cr + C));
        size_t sl = 0, cs = 0;
        wgrad_need(M, C, 9 * C, &sl, &cs);
        w.slab = a.get<float>(sl);
        w.colsum = a.get<float>(cs);
    }
    if (out) *out = w;
    return a.off;
}

bool rcab_dims_ok(int B, int H, int W, int C, int Cr) {
    return B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && Cr >= 1 && Cr <= C && (int64_t)H * W < (1 << 30);
}
int check_rcab(int B, int H, int W, int C, int Cr, const char* who) {
    DCPT_CHECK_ARG(rcab_dims_ok(B, H, W, C, Cr), "%s: B=%d H=%d W=%d C=%d Cr=%d (C must be a positive multiple of 4, 1 <= Cr <= C)", who, B, H,
                   W, C, Cr);
    return DCPT_OK;
}

// ---- upsample stage workspace -------------------------------------------------------------------------
struct PsWs {
    float *wq, *bq;    // weight / bias rows in GEMM column order
    float *wp;         // packed weights: forward [r^2 C][9C], backward [C][9 r^2 C]
    float *dz, *dwq, *dbq;
    float *slab, *colsum;
};

size_t ps_layout(int B, int H, int W, int C, int r, int backward, void* base, size_t bytes, PsWs* out) {
    WsAlloc a(base, bytes);
    PsWs w{};
    const int64_t M = (int64_t)B * H * W;
    const int N = r * r * C;
    w.wq = a.get<float>((size_t)9 * N * C);
    w.wp = a.get<float>((size_t)9 * N * C);
    if (!backward) {
        w.bq = a.get<float>((size_t)N);
    } else {
        w.dz = a.get<float>((size_t)M * N);
        w.dwq = a.get<float>((size_t)9 * N * C);
        w.dbq = a.get<float>((size_t)N);
        size_t sl = 0, cs = 0;
        wgrad_need(M, N, 9 * C, &sl, &cs);
        w.slab = a.get<float>(sl);
        w.colsum = a.get<float>(cs);
    }
    if (out) *out = w;
    return a.off;
}

bool ps_dims_ok(int B, int H, int W, int C, int r) {
    return B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (r == 2 || r == 3) &&
           2.0 * r * H * r * (double)W * C * 4.0 < 1.0e9;   // the fine image fits the scatter epilogue's 32-bit window
}
int check_ps(int B, int H, int W, int C, int r, const char* who) {
    DCPT_CHECK_ARG(ps_dims_ok(B, H, W, C, r),
                   "%s: B=%d H=%d W=%d C=%d r=%d (C a positive multiple of 4, r 2 or 3, one upscaled image below 128 Mi floats)", who, B, H, W,
                   C, r);
    return DCPT_OK;
}

}  // namespace

// the channel-attention kernel on the column sums a conv2 epilogue left (one partial row per (128-row tile, image) pair), for the bf16-storage
// RCAB (rcan_bf16.hip), whose pooled sums, FCs and sigmoid stay fp32: the launch of dcpt_rcab_fwd below
int launch_rcan_ca_fwd(const float* colpart, const float* w1, const float* b1, const float* w2, const float* b2, float* pooled, float* sc, int B,
                       int P, int C, int Cr, hipStream_t s) {
    const int G = dot_groups(C);
    ca_fwd_kernel<<<dim3(B), dim3(256), (size_t)(C + Cr + G * C) * 4, s>>>(colpart, w1, b1, w2, b2, pooled, sc, P, C, Cr, G);
    DCPT_CHECK_LAUNCH("rcab_ca_fwd");
    return DCPT_OK;
}

// =====================================================================================================
extern "C" size_t dcpt_rcab_ws_bytes(int B, int H, int W, int C, int Cr, int backward) {
    if (!rcab_dims_ok(B, H, W, C, Cr)) return 0;
    return rcab_layout(B, H, W, C, Cr, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_rcab_fwd(const dcpt_rcab_params* p, const float* x, float* y, const dcpt_rcab_saved* sv, void* ws, size_t ws_bytes, int B,
                             int H, int W, int C, int Cr, float res_scale, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && x && y && p->conv1_w && p->conv1_b && p->conv2_w && p->conv2_b && p->ca1_w && p->ca1_b && p->ca2_w && p->ca2_b,
                   "rcab_fwd: null argument");
    DCPT_CHECK_ARG(!sv || (sv->h && sv->t && sv->pooled && sv->s), "rcab_fwd: null field in saved (pass saved = NULL to keep nothing)");
    DCPT_TRY(check_rcab(B, H, W, C, Cr, "rcab_fwd"));
    RcabWs w;
    const size_t need = rcab_layout(B, H, W, C, Cr, 0, ws, ws_bytes, &w);
    DCPT_CHECK_WS("rcab_fwd", ws, ws_bytes, need);
    const int P = H * W;
    const int64_t M = (int64_t)B * P;
    float* h = sv ? sv->h : w.h;
    float* t = sv ? sv->t : w.t;
    float* pooled = sv ? sv->pooled : w.pooled;
    float* sc = sv ? sv->s : w.s;
    trace_tag("rcan_rcab_fwd");
    DCPT_TRY(launch_wpack(p->conv1_w, w.wp1, nullptr, C, 9 * C, WP_CONV3, s));
    DCPT_TRY(launch_wpack(p->conv2_w, w.wp2, nullptr, C, 9 * C, WP_CONV3, s));
    // h = relu(conv1(x) + b1)
    GemmNT g = gemm_nt_conv3(x, B, H, W, C, w.wp1, C, h, C);
    g.bias = p->conv1_b;
    DCPT_TRY(launch_gemm_nt(g, A_CONV3, E_RELU, s));
    // t = conv2(h) + b2, and its per-image column sums
    g.A = h; g.Bw = w.wp2; g.C = t; g.bias = p->conv2_b; g.colpart = w.colpart; g.P = P;
    DCPT_TRY(launch_gemm_nt(g, A_CONV3, E_BIASCOL, s));
    const int G = dot_groups(C);
    ca_fwd_kernel<<<dim3(B), dim3(256), (size_t)(C + Cr + G * C) * 4, s>>>(w.colpart, p->ca1_w, p->ca1_b, p->ca2_w, p->ca2_b, pooled, sc, P, C,
                                                                          Cr, G);
    DCPT_CHECK_LAUNCH("rcab_ca_fwd");
    const int64_t n4 = M * C / 4;
    rcab_scale_kernel<<<dim3(ew_grid(n4)), dim3(256), 0, s>>>(reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(t), sc,
                                                              reinterpret_cast<float4*>(y), n4, C, (int64_t)P * C, res_scale);
    DCPT_CHECK_LAUNCH("rcab_scale");
    return DCPT_OK;
}

extern "C" int dcpt_rcab_bwd(const dcpt_rcab_params* p, const dcpt_rcab_params_grads* gr, const float* x, const dcpt_rcab_saved* sv,
                             const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int Cr, float res_scale,
                             dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && gr && x && sv && dy && dx && p->conv1_w && p->conv1_b && p->conv2_w && p->conv2_b && p->ca1_w && p->ca1_b && p->ca2_w &&
                       p->ca2_b,
                   "rcab_bwd: null argument");
    DCPT_CHECK_ARG(sv->h && sv->t && sv->pooled && sv->s, "rcab_bwd: null field in saved");
    DCPT_CHECK_ARG(gr->conv1_w && gr->conv1_b && gr->conv2_w && gr->conv2_b && gr->ca1_w && gr->ca1_b && gr->ca2_w && gr->ca2_b,
                   "rcab_bwd: null gradient");
    DCPT_TRY(check_rcab(B, H, W, C, Cr, "rcab_bwd"));
    RcabWs w;
    const size_t need = rcab_layout(B, H, W, C, Cr, 1, ws, ws_bytes, &w);
    DCPT_CHECK_WS("rcab_bwd", ws, ws_bytes, need);
    const int P = H * W;
    const int64_t M = (int64_t)B * P;
    const int64_t n4 = M * C / 4;
    trace_tag("rcan_rcab_bwd");
    // channel attention: ds = rs sum_hw dy t, its backward, dt = rs dy s + dpooled / P
    const int G = dot_groups(C);
    rcab_dot_kernel<<<dim3(w.ns, B), dim3(256), (size_t)G * C * 4, s>>>(dy, sv->t, w.dpart, P, C, w.ns, cdiv(P, w.ns), G);
    DCPT_CHECK_LAUNCH("rcab_dot");
    ca_bwd_kernel<<<dim3(B), dim3(256), (size_t)(2 * C + 2 * Cr) * 4, s>>>(w.dpart, w.ns, sv->pooled, sv->s, p->ca1_w, p->ca1_b, p->ca2_w,
                                                                          res_scale, w.dpool, w.gp, P, C, Cr);
    DCPT_CHECK_LAUNCH("rcab_ca_bwd");
    ca_grad_reduce_kernel<<<dim3(ew_grid(2 * (int64_t)C * Cr + Cr + C)), dim3(256), 0, s>>>(w.gp, B, C, Cr, gr->ca1_w, gr->ca1_b, gr->ca2_w,
                                                                                          gr->ca2_b);
    DCPT_CHECK_LAUNCH("rcab_ca_grad_reduce");
    rcab_dt_kernel<<<dim3(ew_grid(n4)), dim3(256), 0, s>>>(reinterpret_cast<const float4*>(dy), sv->s, w.dpool, reinterpret_cast<float4*>(w.dt),
                                                           n4, C, (int64_t)P * C, res_scale);
    DCPT_CHECK_LAUNCH("rcab_dt");
    // conv2: dh = [h > 0] conv2^T(dt);  dW2, db2 from dt and h
    DCPT_TRY(launch_conv3_bwd(w.dt, sv->h, p->conv2_w, w.wp2, B, H, W, C, C, E_RELU, sv->h, 0.f, w.dh, w.slab, w.colsum, gr->conv2_w,
                              gr->conv2_b, s));
    // conv1: dx = dy + conv1^T(dh);  dW1, db1 from dh and x
    return launch_conv3_bwd(w.dh, x, p->conv1_w, w.wp1, B, H, W, C, C, E_RESID, dy, 0.f, dx, w.slab, w.colsum, gr->conv1_w, gr->conv1_b, s);
}

// =====================================================================================================
extern "C" size_t dcpt_conv3x3_ps_ws_bytes(int B, int H, int W, int C, int r, int backward) {
    if (!ps_dims_ok(B, H, W, C, r)) return 0;
    return ps_layout(B, H, W, C, r, backward, nullptr, 0, nullptr);
}

extern "C" int dcpt_conv3x3_ps_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H, int W,
                                   int C, int r, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(x && w && bias && y, "conv3x3_ps_fwd: null argument");
    DCPT_TRY(check_ps(B, H, W, C, r, "conv3x3_ps_fwd"));
    PsWs pw;
    const size_t need = ps_layout(B, H, W, C, r, 0, ws, ws_bytes, &pw);
    DCPT_CHECK_WS("conv3x3_ps_fwd", ws, ws_bytes, need);
    const int N = r * r * C;
    trace_tag("rcan_ps_fwd");
    ps_rowperm_kernel<<<dim3(ew_grid((int64_t)N * 9 * C)), dim3(256), 0, s>>>(w, pw.wq, N, 9 * C, C, r, 0);
    DCPT_CHECK_LAUNCH("ps_rowperm");
    ps_rowperm_kernel<<<dim3(ew_grid(N)), dim3(256), 0, s>>>(bias, pw.bq, N, 1, C, r, 0);
    DCPT_CHECK_LAUNCH("ps_rowperm");
    DCPT_TRY(launch_wpack(pw.wq, pw.wp, nullptr, N, 9 * C, WP_CONV3, s));
    GemmNT g = gemm_nt_conv3(x, B, H, W, C, pw.wp, N, y, N);
    g.bias = pw.bq; g.psr = r;
    return launch_gemm_nt(g, A_CONV3, E_PSHUF, s);
}

extern "C" int dcpt_conv3x3_ps_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, void* ws,
                                   size_t ws_bytes, int B, int H, int W, int C, int r, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(dy && x && w && dx && dw && dbias, "conv3x3_ps_bwd: null argument");
    DCPT_TRY(check_ps(B, H, W, C, r, "conv3x3_ps_bwd"));
    PsWs pw;
    const size_t need = ps_layout(B, H, W, C, r, 1, ws, ws_bytes, &pw);
    DCPT_CHECK_WS("conv3x3_ps_bwd", ws, ws_bytes, need);
    const int N = r * r * C;
    const int64_t M = (int64_t)B * H * W;
    trace_tag("rcan_ps_bwd");
    const int64_t n4 = M * N / 4;
    ps_gather_kernel<<<dim3(ew_grid(n4)), dim3(256), 0, s>>>(reinterpret_cast<const float4*>(dy), reinterpret_cast<float4*>(pw.dz), n4, H, W,
                                                             C, r);
    DCPT_CHECK_LAUNCH("ps_gather");
    ps_rowperm_kernel<<<dim3(ew_grid((int64_t)N * 9 * C)), dim3(256), 0, s>>>(w, pw.wq, N, 9 * C, C, r, 0);
    DCPT_CHECK_LAUNCH("ps_rowperm");
    // dx = conv^T(dz): a 3x3 conv of the N-channel map dz with the transposed, flipped weights; the gradients in GEMM column order
    DCPT_TRY(launch_conv3_bwd(pw.dz, x, pw.wq, pw.wp, B, H, W, C, N, E_PLAIN, nullptr, 0.f, dx, pw.slab, pw.colsum, pw.dwq, pw.dbq, s));
    ps_rowperm_kernel<<<dim3(ew_grid((int64_t)N * 9 * C)), dim3(256), 0, s>>>(pw.dwq, dw, N, 9 * C, C, r, 1);
    DCPT_CHECK_LAUNCH("ps_rowperm");
    ps_rowperm_kernel<<<dim3(ew_grid(N)), dim3(256), 0, s>>>(pw.dbq, dbias, N, 1, C, r, 1);
    DCPT_CHECK_LAUNCH("ps_rowperm");
    return DCPT_OK;
}
