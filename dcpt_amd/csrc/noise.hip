// On-the-fly noise of the denoising data path: Gaussian noise here, Poisson (shot) noise on the same Philox stream further down.
// Gaussian (include/dcpt_hip.h dcpt_gauss_noise_fwd): lq = gt + sigma / 255 * n for a batch in
// ONE launch, one read of the batch and one write, no workspace, no atomics, the same bits on every run, and an image's result a function
// of its own (x, sigma, key, gray) alone: the generator is counter-based, so nothing is carried from one element or image to the next.
//
// Generator: Philox4x32-10 (Salmon et al., SC'11), multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, key words
// the low and high half of key[b], counter (q, 0, 0, 0).  Its four outputs x0..x3 give four normals by Box-Muller in fp64:
//     u_i = (x_i + 0.5) 2^-32;   r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2);   n_4q.. = r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3, r1 sin 2 pi u3
// (u > 0, so the logarithm is finite: |n| <= sqrt(66.6 ln 2) = 6.8).  Colour noise: element e of the image's C H W values (NCHW order)
// takes n_e.  Gray noise (gray[b] != 0): pixel p of H W takes n_p in every channel.  y = float(double(x) + double(sigma[b]) / 255 * n), one
// rounding; sigma[b] == 0 hands x through.  CLIP clamps to [0, 1], ROUND8 then takes rint(255 v) / 255 (half to even), ONLY writes the
// noise term without x.
//
// One lane per counter value: four consecutive elements (gray: four consecutive pixels and their C writes).  The image's base b C H W is
// 16-byte aligned only when C H W % 4 == 0 (and a gray plane's only when H W % 4 == 0), so a lane takes the 16-byte load / store where
// its own address allows it and four predicated dwords elsewhere, which also covers the last, partial quad.  In place is allowed: a lane
// reads its elements before it writes them and no other lane touches them.  Bound by the fp64 logarithm / sincos and the ten rounds of
// 32 x 32 -> 64 multiplies, not by memory.
#include <math.h>
#include <stdint.h>

#include "kernels.h"
#include "prof.h"

namespace {
constexpr int NT = 256;
constexpr int MAX_GX = 1 << 16, MAX_GY = 65535;
constexpr int F_CLIP = 1, F_ROUND8 = 2, F_ONLY = 4;   // include/dcpt_hip.h DCPT_NOISE_*

struct NoiseGeom {
    int B, C;
    int64_t plane, chw;   // H W and C H W
    int flags;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

__device__ __forceinline__ double unit(uint32_t v) { return ((double)v + 0.5) * 0x1p-32; }

__device__ __forceinline__ float finish(double v, int flags) {
    if (flags & F_CLIP) v = fmin(fmax(v, 0.0), 1.0);
    if (flags & F_ROUND8) v = rint(255.0 * v) / 255.0;
    return (float)v;
}

__global__ __launch_bounds__(NT) void gauss_noise_kernel(const float* x, const float* __restrict__ sigma, const long long* __restrict__ key,
                                                         const int* __restrict__ gray, float* y, NoiseGeom m) {
    const bool only = (m.flags & F_ONLY) != 0;
    for (int b = blockIdx.y; b < m.B; b += gridDim.y) {
        const bool g = gray != nullptr && gray[b] != 0;
        const int64_t n = g ? m.plane : m.chw;   // the values of this image's stream
        const int64_t nq = (n + 3) >> 2;         // below 2^32: the counter's first word holds q
        const float sg = sigma[b];
        const double s = (double)sg / 255.0;
        const bool pass = sg == 0.0f && m.flags == 0;   // x bit for bit, a negative zero included
        const uint64_t k = (uint64_t)key[b];
        const int reps = g ? m.C : 1;
        for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < nq; q += (int64_t)gridDim.x * NT) {
            uint32_t r[4];
            philox4x32_10((uint32_t)q, (uint32_t)k, (uint32_t)(k >> 32), r);
            const double r0 = sqrt(-2.0 * log(unit(r[0]))), r1 = sqrt(-2.0 * log(unit(r[2])));
            double s0, c0, s1, c1;
            sincospi(2.0 * unit(r[1]), &s0, &c0);
            sincospi(2.0 * unit(r[3]), &s1, &c1);
            const double t[4] = {s * (r0 * c0), s * (r0 * s0), s * (r1 * c1), s * (r1 * s1)};
            const int64_t e0 = q << 2;
            const bool full = e0 + 4 <= n;
            for (int c = 0; c < reps; ++c) {
                const int64_t off = (int64_t)b * m.chw + c * m.plane + e0;
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (!only) {
                    const float* xp = x + off;
                    if (full && ((uintptr_t)xp & 15) == 0) {
                        const float4 w = *reinterpret_cast<const float4*>(xp);
                        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (e0 + j < n) v[j] = xp[j];
                    }
                }
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = pass ? v[j] : finish((double)v[j] + t[j], m.flags);
                float* yp = y + off;
                if (full && ((uintptr_t)yp & 15) == 0) {
                    *reinterpret_cast<float4*>(yp) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (e0 + j < n) yp[j] = o[j];
                }
            }
        }
    }
}

// ---- Poisson (shot) noise (include/dcpt_hip.h dcpt_poisson_noise_fwd) -----------------------------------------------------------------
// Two launches.  poisson_levels_kernel: grid (chunks, B); a workgroup ORs the presence bits of the 8-bit levels of its share of an image
// (8 words per lane, a wave-wide OR by shuffles, the four waves through LDS) and stores ONE 256-bit mask per (image, chunk) with plain
// stores: no atomics, and an OR does not care how the image was cut.  The chunk count is the same for every image of a call,
// min(32, ceil(C H W / 4096)) (a gray image has fewer values; its surplus chunks store empty masks), so the sampler ORs at most 32 masks.
// poisson_noise_kernel: the addressing of gauss_noise_kernel (one lane per counter value: four elements, or four pixels and their C
// writes).  Per image a block ORs the masks, counts the bits, derives vals and fills exp(-lambda_l) for the 256 levels in LDS; R[k] = 1 / k
// is filled once per block.  A lane then runs the upward search for its four values in lockstep (one k for the four, so one broadcast
// LDS read of R[k] per step); a wave runs to the largest k of its 256 values.  Every fp64 product and sum is rounded on its own.
constexpr int LEVEL_CHUNK = 4096, MAX_CHUNKS = 32, KCAP = 1023;
constexpr int PROF_POISSON_LEVELS = PROF_OTHER + 8, PROF_POISSON_SAMPLE = PROF_OTHER + 9;   // class ids of dcpt_prof_read's rows

__device__ __forceinline__ int level_of(double v) { return (int)fmin(fmax(rint(255.0 * v), 0.0), 255.0); }   // NaN -> 0

__device__ __forceinline__ double gray_of(float r, float g, float b) {
#pragma clang fp contract(off)   // each product and sum rounded on its own
    return (0.2989 * (double)r + 0.587 * (double)g) + 0.114 * (double)b;
}

__global__ __launch_bounds__(NT) void poisson_levels_kernel(const float* __restrict__ x, const int* __restrict__ gray, uint32_t* __restrict__ masks,
                                                            NoiseGeom m) {
    __shared__ uint32_t part[NT / 64][8];
    const int nch = gridDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = blockIdx.y; b < m.B; b += gridDim.y) {
        const bool g = gray != nullptr && gray[b] != 0;
        const int64_t n = g ? m.plane : m.chw;
        const float* xb = x + (int64_t)b * m.chw;
        uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)nch * NT) {
            const double v = (g && m.C == 3) ? gray_of(xb[e], xb[m.plane + e], xb[2 * m.plane + e]) : (double)xb[e];
            const int l = level_of(v);
            const uint32_t bit = 1u << (l & 31);
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] |= (l >> 5) == j ? bit : 0u;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) w[j] |= __shfl_xor(w[j], d, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) part[wave][j] = w[j];
        }
        __syncthreads();
        if (threadIdx.x < 8) {
            uint32_t o = 0u;
#pragma unroll
            for (int k = 0; k < NT / 64; ++k) o |= part[k][threadIdx.x];
            masks[((int64_t)b * nch + blockIdx.x) * 8 + threadIdx.x] = o;
        }
        __syncthreads();   // (part is rewritten for the next image of this block)
    }
}

__global__ __launch_bounds__(NT) void poisson_noise_kernel(const float* x, const float* __restrict__ scale, const long long* __restrict__ key,
                                                           const int* __restrict__ gray, float* y, const uint32_t* __restrict__ masks,
                                                           int* __restrict__ vals_out, int nch, NoiseGeom m) {
    // Every fp64 product and sum of the sampler is rounded on its own.  Plain operators under this pragma: the __dmul_rn / __dadd_rn of the
    // HIP headers are inline functions compiled under the default contraction mode, and the compiler fused them into v_fmac_f64 here.
#pragma clang fp contract(off)
    __shared__ double s_exp[256];        // exp(-lambda_l) of the image at hand
    __shared__ double s_rcp[KCAP + 1];   // R[k] = 1 / k (R[0] unused)
    __shared__ int s_cnt[8];
    const bool only = (m.flags & F_ONLY) != 0;
    for (int k = threadIdx.x; k <= KCAP; k += NT) s_rcp[k] = k ? 1.0 / (double)k : 0.0;
    for (int b = blockIdx.y; b < m.B; b += gridDim.y) {
        if (threadIdx.x < 8) {
            uint32_t o = 0u;
            for (int c = 0; c < nch; ++c) o |= masks[((int64_t)b * nch + c) * 8 + threadIdx.x];
            s_cnt[threadIdx.x] = __popc(o);
        }
        __syncthreads();
        int U = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) U += s_cnt[j];
        int vals = 1;
        while (vals < U) vals <<= 1;   // U is 1..256
        if (blockIdx.x == 0 && threadIdx.x == 0) vals_out[b] = vals;
        const double dvals = (double)vals;
        s_exp[threadIdx.x] = exp(-((double)(threadIdx.x * vals) / 255.0));   // (NT == 256: one level per lane)
        __syncthreads();

        const bool g = gray != nullptr && gray[b] != 0;
        const int64_t n = g ? m.plane : m.chw;
        const int64_t nq = (n + 3) >> 2;
        const float sc = scale[b];
        const double s = (double)sc;
        const bool pass = sc == 0.0f && m.flags == 0;   // x bit for bit
        const uint64_t kw = (uint64_t)key[b];
        const int reps = g ? m.C : 1;                   // 1 or 3 (the entry point refuses a gray flag array with another C)
        for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < nq; q += (int64_t)gridDim.x * NT) {
            const int64_t e0 = q << 2;
            const bool full = e0 + 4 <= n;
            float v[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[c][j] = 0.0f;
                if (c < reps) {
                    const float* xp = x + (int64_t)b * m.chw + c * m.plane + e0;
                    if (full && ((uintptr_t)xp & 15) == 0) {
                        const float4 w = *reinterpret_cast<const float4*>(xp);
                        v[c][0] = w.x; v[c][1] = w.y; v[c][2] = w.z; v[c][3] = w.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (e0 + j < n) v[c][j] = xp[j];
                    }
                }
            }
            double t[4] = {0.0, 0.0, 0.0, 0.0};
            if (!pass) {
                uint32_t r[4];
                philox4x32_10((uint32_t)q, (uint32_t)kw, (uint32_t)(kw >> 32), r);
                double u[4], lam[4], p[4], acc[4];
                int lev[4], kk[4] = {0, 0, 0, 0};
                bool act[4];
                bool any = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lev[j] = level_of(reps == 3 ? gray_of(v[0][j], v[1][j], v[2][j]) : (double)v[0][j]);
                    lam[j] = (double)(lev[j] * vals) / 255.0;
                    u[j] = e0 + j < n ? unit(r[j]) : 0.0;   // (a value past the end never searches)
                    p[j] = s_exp[lev[j]];
                    acc[j] = p[j];
                    act[j] = acc[j] < u[j];
                    any |= act[j];
                }
                // The four searches step together and without a branch.  A sum never decreases (p >= 0), so a value whose sum has reached
                // its u stays there while the others go on: its recurrence may run on unread, and k is the number of steps that began
                // with s < u -- the k of the loop in the header.
                for (int k = 1; any && k <= KCAP; ++k) {
                    const double rk = s_rcp[k];
                    any = false;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        p[j] = (p[j] * lam[j]) * rk;
                        acc[j] = acc[j] + p[j];
                        kk[j] += act[j] ? 1 : 0;
                        act[j] = acc[j] < u[j];
                        any |= act[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = s * ((double)kk[j] / dvals - (double)lev[j] / 255.0);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c < reps) {
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = pass ? v[c][j] : finish(only ? t[j] : (double)v[c][j] + t[j], m.flags);
                    float* yp = y + (int64_t)b * m.chw + c * m.plane + e0;
                    if (full && ((uintptr_t)yp & 15) == 0) {
                        *reinterpret_cast<float4*>(yp) = make_float4(o[0], o[1], o[2], o[3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (e0 + j < n) yp[j] = o[j];
                    }
                }
            }
        }
        __syncthreads();   // (s_cnt and s_exp are rewritten for the next image of this block)
    }
}

int poisson_chunks(int64_t chw) {
    const int64_t c = cdiv64(chw, LEVEL_CHUNK);
    return (int)(c < MAX_CHUNKS ? c : MAX_CHUNKS);
}
size_t poisson_vals_bytes(int B) { return align_up((size_t)B * sizeof(int), 256); }
}  // namespace

size_t poisson_noise_ws_bytes(int B, int C, int H, int W) {
    return poisson_vals_bytes(B) + align_up((size_t)B * poisson_chunks((int64_t)C * H * W) * 8 * sizeof(uint32_t), 256);
}

int launch_poisson_noise_fwd(const float* x, const float* scale, const long long* key, const int* gray, float* y, void* ws, int B, int C, int H,
                             int W, int flags, hipStream_t s) {
    NoiseGeom m{};
    m.B = B; m.C = C;
    m.plane = (int64_t)H * W;
    m.chw = m.plane * C;
    m.flags = flags;
    int* vals = (int*)ws;
    uint32_t* masks = (uint32_t*)((char*)ws + poisson_vals_bytes(B));
    const int nch = poisson_chunks(m.chw);
    const unsigned gy = (unsigned)(B < MAX_GY ? B : MAX_GY);
    const double bytes = 4.0 * (double)B * (double)m.chw;
    {
        ProfScope prof(s, PROF_POISSON_LEVELS, (int64_t)B * m.chw, 0, 0, 0.0, bytes);   // (launch timing, off by default: dcpt_prof_enable)
        trace_tag("noise.poisson_levels");
        poisson_levels_kernel<<<dim3((unsigned)nch, gy), dim3(NT), 0, s>>>(x, gray, masks, m);
        DCPT_CHECK_LAUNCH("poisson_noise_fwd (levels)");
    }
    const int64_t gx = cdiv64((m.chw + 3) >> 2, NT);
    ProfScope prof(s, PROF_POISSON_SAMPLE, (int64_t)B * m.chw, 0, 0, 0.0, 2.0 * bytes);
    trace_tag("noise.poisson");
    poisson_noise_kernel<<<dim3((unsigned)(gx < MAX_GX ? gx : MAX_GX), gy), dim3(NT), 0, s>>>(x, scale, key, gray, y, masks, vals, nch, m);
    DCPT_CHECK_LAUNCH("poisson_noise_fwd");
    return DCPT_OK;
}

int launch_gauss_noise_fwd(const float* x, const float* sigma, const long long* key, const int* gray, float* y, int B, int C, int H, int W,
                           int flags, hipStream_t s) {
    NoiseGeom m{};
    m.B = B; m.C = C;
    m.plane = (int64_t)H * W;
    m.chw = m.plane * C;
    m.flags = flags;
    const int64_t nq = (m.chw + 3) >> 2;   // a colour image's quads; a gray image uses the first ceil(H W / 4) lanes of them
    const int64_t gx = cdiv64(nq, NT);
    const dim3 grid((unsigned)(gx < MAX_GX ? gx : MAX_GX), (unsigned)(B < MAX_GY ? B : MAX_GY)), block(NT);
    trace_tag("noise.gauss");
    gauss_noise_kernel<<<grid, block, 0, s>>>(x, sigma, key, gray, y, m);
    DCPT_CHECK_LAUNCH("gauss_noise_fwd");
    return DCPT_OK;
}
