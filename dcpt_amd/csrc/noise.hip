// On-the-fly Gaussian noise of the denoising data path (include/dcpt_hip.h dcpt_gauss_noise_fwd): lq = gt + sigma / 255 * n for a batch in
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
}  // namespace

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
