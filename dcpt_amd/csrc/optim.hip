// AdamW over a LIST of fp32 parameter tensors in a few launches (the optimizer step that closes every training step of the path:
// reference basicsr/models/base_model.py:70-93 builds torch.optim.AdamW, sr_model.py:118 / degradation_classification_pretrain_model.py:170-173
// call optimizer.step()).  The update is elementwise and purely bandwidth-bound -- 4 reads + 3 writes of 4 bytes per parameter, 1.9 GB for
// the 67.9 M parameters of NAFNet-64 [1,1,1,28] -- and the network has 664 parameter tensors, most of them 64 .. 2048 elements: torch's
// fused kernel takes 36 tensors and 320 blocks per launch (19-23 launches, 1.7 ms for that network); here a launch takes AW_MAX tensors
// whatever their sizes, their pointers travel in the kernel arguments (no device-side table, no copy), a block owns one 4096-element chunk
// of one tensor and finds it by a binary search over the per-tensor block offsets.
//
// Arithmetic (per element, fp32, the order of torch's _fused_adamw_ kernel):
//     p -= lr wd p;   m = lerp(m, g, 1 - b1);   v = b2 v + (1 - b2) g g;   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// with bc1 = 1 - b1^t, bc2 = 1 - b2^t computed by the caller in double precision.
//
// The step tail around it (reference sr_model.py:166-174 clip_grad_norm_ -> optimizer.step() -> model_ema(), base_model.py:86-95) rides on
// the same block map: gradnorm_kernel reads every gradient once and leaves one fp64 sum of squares per block, gradnorm_finish_kernel turns
// them into {norm, clip coefficient} in device memory, and adamw_kernel<CLIP, EMA> multiplies the gradient by that coefficient while it
// has it in registers and updates the EMA copy while it has the new parameter in registers: 10 passes of 4 bytes per parameter instead of
// the 15 of clip_grad_norm_ + step + two foreach passes, no host read-back.  adamw_kernel<false, false> is the plain step, unchanged.
#include "dcpt_common.h"
#include "../../include/dcpt_hip.h"
#include "prof.h"
#include <type_traits>

namespace {

constexpr int AW_MAX = 80;       // tensors per launch: 80 x (4 pointers + size + offset) = 3.2 KB of kernel arguments
constexpr int AW_CHUNK = 4096;   // elements per block: 256 threads x 4 float4

struct AdamWArgs {
    float* p[AW_MAX];
    const float* g[AW_MAX];
    float* m[AW_MAX];
    float* v[AW_MAX];
    uint32_t n[AW_MAX];
    uint32_t blk0[AW_MAX + 1];   // first block of tensor i; blk0[cnt] = number of blocks
    int cnt;
    float lr_wd, w1, b2, omb2, step_size, bc2_sqrt, eps, gsign;
};

struct AdamWArgsEx : AdamWArgs {   // the CLIP / EMA forms: one more pointer per tensor and the two device-side scalars
    float* e[AW_MAX];
    const float* coef;   // CLIP: the clip coefficient gradnorm_finish_kernel left in device memory
    float decay, omd;    // EMA: e = e decay + (1 - decay) p
};
static_assert(sizeof(AdamWArgs) <= 4096 && sizeof(AdamWArgsEx) <= 4096, "the tensor table travels as a by-value kernel argument");

struct GradNormArgs {
    const float* g[AW_MAX];
    uint32_t n[AW_MAX];
    uint32_t blk0[AW_MAX + 1];
    int cnt;
    double* partials;   // of this launch: partials[blockIdx.x]
};
static_assert(sizeof(GradNormArgs) <= 4096, "the tensor table travels as a by-value kernel argument");

__device__ __forceinline__ float lerp_t(float a, float b, float w) {   // at::native::lerp (weight < 0.5 ? a + w (b - a) : b - (b - a)(1 - w))
    const float d = b - a;
    return w < 0.5f ? a + w * d : b - d * (1.0f - w);
}

// torch's _foreach_mul_(e, decay); _foreach_add_(e, p, alpha = 1 - decay): the product rounds, the add contracts into an FMA
__device__ __forceinline__ float ema_one(float e, float p, float decay, float omd) { return __fmaf_rn(omd, p, __fmul_rn(e, decay)); }

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamWArgs& a) {
    g *= a.gsign;
    p -= a.lr_wd * p;
    m = lerp_t(m, g, a.w1);
    v = a.b2 * v + a.omb2 * g * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;   // (a division, as torch's fused kernel: the kernel is bandwidth-bound, and a resumed run reproduces bit for bit)
    p -= a.step_size * m / denom;
}

template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(const typename std::conditional<CLIP || EMA, AdamWArgsEx, AdamWArgs>::type args) {
    const AdamWArgs& a = args;
    // tensor of this block: the last i with blk0[i] <= blockIdx.x (wave-uniform: scalar loads from the kernel arguments)
    int lo = 0, hi = a.cnt - 1;
    const uint32_t b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.blk0[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t n = a.n[lo];
    const uint32_t e0 = (b - a.blk0[lo]) * (uint32_t)AW_CHUNK;
    float* __restrict__ P = a.p[lo];
    const float* __restrict__ G = a.g[lo];
    float* __restrict__ M = a.m[lo];
    float* __restrict__ V = a.v[lo];
    float* __restrict__ E = nullptr;
    float coef = 1.0f, decay = 0.0f, omd = 0.0f;
    if constexpr (CLIP) coef = *args.coef;   // (wave-uniform: one scalar load)
    if constexpr (EMA) {
        E = args.e[lo];
        decay = args.decay;
        omd = args.omd;
    }
    const bool vec = (((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V | (uintptr_t)E) & 15) == 0;
    if (vec && e0 + AW_CHUNK <= n) {
        float4 pv[4], gv[4], mv[4], vv[4], ev[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // all sixteen loads in flight before the first use
            const uint32_t e = e0 + (uint32_t)(j * 256 + threadIdx.x) * 4u;
            pv[j] = *reinterpret_cast<const float4*>(P + e);
            gv[j] = *reinterpret_cast<const float4*>(G + e);
            mv[j] = *reinterpret_cast<const float4*>(M + e);
            vv[j] = *reinterpret_cast<const float4*>(V + e);
            if constexpr (EMA) ev[j] = *reinterpret_cast<const float4*>(E + e);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t e = e0 + (uint32_t)(j * 256 + threadIdx.x) * 4u;
            if constexpr (CLIP) {
                gv[j].x *= coef; gv[j].y *= coef; gv[j].z *= coef; gv[j].w *= coef;
            }
            adamw_one(pv[j].x, gv[j].x, mv[j].x, vv[j].x, a);
            adamw_one(pv[j].y, gv[j].y, mv[j].y, vv[j].y, a);
            adamw_one(pv[j].z, gv[j].z, mv[j].z, vv[j].z, a);
            adamw_one(pv[j].w, gv[j].w, mv[j].w, vv[j].w, a);
            *reinterpret_cast<float4*>(P + e) = pv[j];
            *reinterpret_cast<float4*>(M + e) = mv[j];
            *reinterpret_cast<float4*>(V + e) = vv[j];
            if constexpr (EMA) {
                ev[j].x = ema_one(ev[j].x, pv[j].x, decay, omd);
                ev[j].y = ema_one(ev[j].y, pv[j].y, decay, omd);
                ev[j].z = ema_one(ev[j].z, pv[j].z, decay, omd);
                ev[j].w = ema_one(ev[j].w, pv[j].w, decay, omd);
                *reinterpret_cast<float4*>(E + e) = ev[j];
            }
        }
    } else {   // a tensor's last chunk, tensors shorter than a chunk, views that are not 16-byte aligned
        for (uint32_t e = e0 + threadIdx.x; e < n && e < e0 + AW_CHUNK; e += 256) {
            float p = P[e], m = M[e], v = V[e], g = G[e];
            if constexpr (CLIP) g *= coef;
            adamw_one(p, g, m, v, a);
            P[e] = p;
            M[e] = m;
            V[e] = v;
            if constexpr (EMA) E[e] = ema_one(E[e], p, decay, omd);
        }
    }
}

// Sum of squares of a list of gradients: adamw_kernel's block map, every thread accumulates in fp64 (the kernel is bandwidth-bound; fp64
// removes the overflow and the order sensitivity of a 68 M-term fp32 sum), one double per block, no atomics: the result does not depend
// on scheduling.
__device__ __forceinline__ double block_sum_f64(double s, double* red) {   // 256 threads = 4 waves of 64; valid in thread 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void gradnorm_kernel(const GradNormArgs a) {
    __shared__ double red[4];
    int lo = 0, hi = a.cnt - 1;
    const uint32_t b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.blk0[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t n = a.n[lo];
    const uint32_t e0 = (b - a.blk0[lo]) * (uint32_t)AW_CHUNK;
    const float* __restrict__ G = a.g[lo];
    double s = 0.0;
    if (((uintptr_t)G & 15) == 0 && e0 + AW_CHUNK <= n) {
        float4 gv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = *reinterpret_cast<const float4*>(G + e0 + (uint32_t)(j * 256 + threadIdx.x) * 4u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double x = gv[j].x, y = gv[j].y, z = gv[j].z, w = gv[j].w;
            s += x * x;
            s += y * y;
            s += z * z;
            s += w * w;
        }
    } else {
        for (uint32_t e = e0 + threadIdx.x; e < n && e < e0 + AW_CHUNK; e += 256) {
            const double x = G[e];
            s += x * x;
        }
    }
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) a.partials[b] = s;
}

// {norm, coefficient} of torch.nn.utils.clip_grad_norm_ (error_if_nonfinite=False): the partial sums in a fixed strided order in fp64, one
// rounding to fp32 after the square root, then torch's fp32 arithmetic.  (c > 1 ? 1 : c) keeps a NaN norm a NaN coefficient, as
// torch.clamp(max=1) does; fminf would turn it into 1.
__global__ __launch_bounds__(256) void gradnorm_finish_kernel(const double* __restrict__ partials, uint32_t count, float max_norm, float* __restrict__ out2) {
    __shared__ double red[4];
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < count; i += 256) s += partials[i];
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const float c = max_norm / (norm + 1e-6f);
        out2[0] = norm;
        out2[1] = (c > 1.0f) ? 1.0f : c;
    }
}

int64_t gradnorm_blocks(int n, const int64_t* numel) {   // -1: a count out of range
    int64_t blocks = 0;
    for (int k = 0; k < n; ++k) {
        if (numel[k] < 0 || numel[k] >= ((int64_t)1 << 32) - AW_CHUNK) return -1;
        blocks += (numel[k] + AW_CHUNK - 1) / AW_CHUNK;
    }
    return blocks;
}

template <bool CLIP, bool EMA>
int adamw_launch(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, float* const* ema,
                 const int64_t* numel, const dcpt_adamw_hparams* h, const float* clip_coef, double ema_decay, hipStream_t s) {
    int64_t total = 0;
    for (int k = 0; k < n; ++k) total += numel[k] > 0 ? numel[k] : 0;
    ProfScope prof(s, PROF_OTHER + 4, total, 0, 0, 12.0 * (double)total, (EMA ? 36.0 : 28.0) * (double)total);
    typename std::conditional<CLIP || EMA, AdamWArgsEx, AdamWArgs>::type a{};
    a.lr_wd = (float)(h->lr * h->weight_decay);
    a.w1 = (float)(1.0 - h->beta1);
    a.b2 = (float)h->beta2;
    a.omb2 = (float)(1.0 - h->beta2);
    a.step_size = (float)(h->lr / h->bias_correction1);
    a.bc2_sqrt = (float)sqrt(h->bias_correction2);
    a.eps = (float)h->eps;
    a.gsign = h->maximize ? -1.0f : 1.0f;
    if constexpr (CLIP) a.coef = clip_coef;
    if constexpr (EMA) {
        a.decay = (float)ema_decay;
        a.omd = (float)(1.0 - ema_decay);
    }
    // every check before the first launch: a bad tensor late in the list must not leave the first 80 stepped
    for (int k = 0; k < n; ++k) {
        if (numel[k] == 0) continue;
        DCPT_CHECK_ARG(numel[k] > 0 && numel[k] < ((int64_t)1 << 32) - AW_CHUNK, "adamw_step: tensor %d has %lld elements (1 .. 2^32 - 4097)", k,
                       (long long)numel[k]);
        DCPT_CHECK_ARG(params[k] && grads[k] && exp_avg[k] && exp_avg_sq[k] && (!EMA || ema[k]), "adamw_step: tensor %d has a null pointer", k);
    }
    int i = 0;
    while (i < n) {
        a.cnt = 0;
        uint32_t blocks = 0;
        for (; i < n && a.cnt < AW_MAX; ++i) {
            if (numel[i] == 0) continue;
            a.p[a.cnt] = params[i]; a.g[a.cnt] = grads[i]; a.m[a.cnt] = exp_avg[i]; a.v[a.cnt] = exp_avg_sq[i];
            if constexpr (EMA) a.e[a.cnt] = ema[i];
            a.n[a.cnt] = (uint32_t)numel[i];
            a.blk0[a.cnt] = blocks;
            blocks += (uint32_t)((numel[i] + AW_CHUNK - 1) / AW_CHUNK);
            ++a.cnt;
        }
        if (a.cnt == 0) break;
        a.blk0[a.cnt] = blocks;
        trace_tag(CLIP && EMA ? "adamw.clip_ema" : CLIP ? "adamw.clip" : EMA ? "adamw.ema" : "adamw");
        adamw_kernel<CLIP, EMA><<<dim3(blocks), dim3(256), 0, s>>>(a);
        DCPT_CHECK_LAUNCH("adamw");
    }
    return DCPT_OK;
}

int adamw_check(const char* who, int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                const int64_t* numel, const dcpt_adamw_hparams* h) {
    DCPT_CHECK_ARG(n >= 0 && (n == 0 || (params && grads && exp_avg && exp_avg_sq && numel)) && h, "%s: null argument", who);
    DCPT_CHECK_ARG(h->bias_correction1 > 0.0 && h->bias_correction2 > 0.0 && h->beta1 >= 0.0 && h->beta1 < 1.0 && h->beta2 >= 0.0 && h->beta2 < 1.0,
                   "%s: betas in [0, 1) and positive bias corrections (step >= 1) expected", who);
    return DCPT_OK;
}

}  // namespace

extern "C" int dcpt_adamw_step(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                               const int64_t* numel, const dcpt_adamw_hparams* h, dcpt_stream_t stream) {
    DCPT_TRY(adamw_check("adamw_step", n, params, grads, exp_avg, exp_avg_sq, numel, h));
    return adamw_launch<false, false>(n, params, grads, exp_avg, exp_avg_sq, nullptr, numel, h, nullptr, 0.0, (hipStream_t)stream);
}

extern "C" int dcpt_adamw_step_ex(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                  float* const* ema, const int64_t* numel, const dcpt_adamw_hparams* h, const float* clip_coef,
                                  double ema_decay, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_TRY(adamw_check("adamw_step_ex", n, params, grads, exp_avg, exp_avg_sq, numel, h));
    DCPT_CHECK_ARG(!ema || (ema_decay >= 0.0 && ema_decay <= 1.0), "adamw_step_ex: ema_decay %g outside [0, 1]", ema_decay);
    if (clip_coef && ema) return adamw_launch<true, true>(n, params, grads, exp_avg, exp_avg_sq, ema, numel, h, clip_coef, ema_decay, s);
    if (clip_coef) return adamw_launch<true, false>(n, params, grads, exp_avg, exp_avg_sq, nullptr, numel, h, clip_coef, 0.0, s);
    if (ema) return adamw_launch<false, true>(n, params, grads, exp_avg, exp_avg_sq, ema, numel, h, nullptr, ema_decay, s);
    return adamw_launch<false, false>(n, params, grads, exp_avg, exp_avg_sq, nullptr, numel, h, nullptr, 0.0, s);
}

extern "C" size_t dcpt_grad_norm_ws_bytes(int n, const int64_t* numel) {
    if (n <= 0 || !numel) return 0;
    const int64_t blocks = gradnorm_blocks(n, numel);
    return blocks < 0 ? 0 : (size_t)blocks * sizeof(double);
}

extern "C" int dcpt_grad_norm(int n, const float* const* grads, const int64_t* numel, float max_norm, void* workspace, size_t workspace_bytes,
                              float* out2, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(n >= 0 && (n == 0 || (grads && numel)) && out2, "grad_norm: null argument");
    for (int k = 0; k < n; ++k) {
        DCPT_CHECK_ARG(numel[k] >= 0 && numel[k] < ((int64_t)1 << 32) - AW_CHUNK, "grad_norm: tensor %d has %lld elements (0 .. 2^32 - 4097)", k,
                       (long long)numel[k]);
        DCPT_CHECK_ARG(numel[k] == 0 || grads[k], "grad_norm: tensor %d has a null pointer", k);
    }
    const int64_t total_blocks = gradnorm_blocks(n, numel);
    DCPT_CHECK_ARG(total_blocks < ((int64_t)1 << 32), "grad_norm: %lld blocks", (long long)total_blocks);
    if ((size_t)total_blocks * sizeof(double) > workspace_bytes || (total_blocks > 0 && !workspace)) {
        dcpt_set_error("grad_norm: workspace too small or null (%zu bytes given, %zu needed)", workspace ? workspace_bytes : (size_t)0,
                       (size_t)total_blocks * sizeof(double));
        return DCPT_ERR_WS;
    }
    double* partials = (double*)workspace;
    GradNormArgs a{};
    uint32_t done = 0;
    int i = 0;
    while (i < n) {
        a.cnt = 0;
        uint32_t blocks = 0;
        for (; i < n && a.cnt < AW_MAX; ++i) {
            if (numel[i] == 0) continue;
            a.g[a.cnt] = grads[i];
            a.n[a.cnt] = (uint32_t)numel[i];
            a.blk0[a.cnt] = blocks;
            blocks += (uint32_t)((numel[i] + AW_CHUNK - 1) / AW_CHUNK);
            ++a.cnt;
        }
        if (a.cnt == 0) break;
        a.blk0[a.cnt] = blocks;
        a.partials = partials + done;
        trace_tag("grad_norm.sumsq");
        gradnorm_kernel<<<dim3(blocks), dim3(256), 0, s>>>(a);
        DCPT_CHECK_LAUNCH("grad_norm");
        done += blocks;
    }
    trace_tag("grad_norm.finish");
    gradnorm_finish_kernel<<<dim3(1), dim3(256), 0, s>>>(partials, done, max_norm, out2);
    DCPT_CHECK_LAUNCH("grad_norm_finish");
    return DCPT_OK;
}
