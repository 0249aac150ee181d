// Synthetic blur of the blur data path (include/dcpt_hip.h dcpt_filter2d_fwd): y = the K x K correlation (no flip) of every plane of x,
// reflect-padded by r = K / 2, with its image's kernel; ONE launch, one read of the batch and one write, no workspace, no atomics, the same
// bits on every run.  Replaces the reference's filter2D (basicsr/utils/img_process_util.py:7-31: F.pad + a grouped F.conv2d).
//
// Arithmetic, per output element: acc = 0.0; for dy = 0 .. K - 1, for dx = 0 .. K - 1: acc = fma((double)kern[dy][dx], (double)x[..], acc);
// y = (float)acc.  The product of two fp32 values is exact in fp64, so each step rounds once whether or not it is contracted, and the sum
// has one value.  It is NOT split: one accumulator per output walks the K * K taps in that order.
//
// One workgroup of 256 owns a 32 x 64 output tile of one (b, c) plane.  LDS: the image's K * K taps as doubles (converted once) and the
// tile with its halo, (32 + K - 1) rows of fp32, reflected while loading (-i -> i, H - 1 + i -> H - 1 - i; the halo of a ragged tile beyond
// that is clamped and never used).  A lane owns 2 rows x 4 columns of outputs in eight fp64 accumulators and walks the tile rows r0 .. r0 + K:
// row r0 + t is tap row t of its upper outputs and tap row t - 1 of its lower ones, so one row segment read from LDS feeds both, and a
// segment is read as 16-byte words (4 columns), each value feeding up to 8 FMAs; a tap is one 8-byte broadcast read per 4 FMAs.  The 16
// lanes along W read 64 consecutive dwords and the row pitch is a multiple of 32 dwords, so the lanes of a 16-byte read that lie in
// different rows (rows 2 apart: a multiple of 64 dwords) hit disjoint banks.  At K = 51: 20.8 KB of taps + 82 x 128 x 4 = 42 KB of tile.
#include <math.h>
#include <stdint.h>

#include "kernels.h"
#include "prof.h"

namespace {
constexpr int NT = 256;
constexpr int TW = 64, TH = 32;           // the output tile
constexpr int PX = 4, PY = 2;             // outputs per lane along W and H
constexpr int LANES_X = TW / PX;          // 16 lanes along W, NT / 16 = 16 along H
static_assert(LANES_X * (TH / PY) == NT, "one lane per 2 x 4 outputs");

struct BlurGeom {
    int C, H, W, K;
    int per_image;
    int gx, tiles;    // tiles per row of tiles, tiles per plane
    int pitch;        // dwords per LDS tile row
    int tap_bytes;    // the taps' share of LDS
};

// the padded coordinate brought into the plane: the reflection for -r .. n - 1 + r (r < n), a clamp for whatever a ragged tile adds
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return min(max(i, 0), n - 1);
}

// ND taps dx0 .. dx0 + ND - 1 of one tile row: w[0 .. 7] holds the row's columns c0 + dx0 .. c0 + dx0 + 7
template <bool UP, bool LO, int ND>
__device__ __forceinline__ void taps(const double* __restrict__ ku, const double* __restrict__ kl, int dx0, const double (&w)[8],
                                     double (&acc)[PY][PX]) {
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        if (UP) {
            const double kv = ku[dx0 + d];
#pragma unroll
            for (int j = 0; j < PX; ++j) acc[0][j] = fma(kv, w[j + d], acc[0][j]);
        }
        if (LO) {
            const double kv = kl[dx0 + d];
#pragma unroll
            for (int j = 0; j < PX; ++j) acc[1][j] = fma(kv, w[j + d], acc[1][j]);
        }
    }
}

// one tile row: tap row ku of the upper outputs (UP) and kl of the lower ones (LO), dx ascending
template <bool UP, bool LO>
__device__ __forceinline__ void tile_row(const float* __restrict__ row, const double* __restrict__ ku, const double* __restrict__ kl, int K,
                                         double (&acc)[PY][PX]) {
    const float4* q = reinterpret_cast<const float4*>(row);
    double w[8];
    float4 f = q[0];
    w[0] = f.x; w[1] = f.y; w[2] = f.z; w[3] = f.w;
    const int full = K >> 2;
    int c = 0;
    for (; c < full; ++c) {
        f = q[c + 1];
        w[4] = f.x; w[5] = f.y; w[6] = f.z; w[7] = f.w;
        taps<UP, LO, 4>(ku, kl, 4 * c, w, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = w[j + 4];
    }
    f = q[c + 1];
    w[4] = f.x; w[5] = f.y; w[6] = f.z; w[7] = f.w;
    if ((K & 3) == 1) taps<UP, LO, 1>(ku, kl, 4 * c, w, acc);   // K is odd: one or three taps are left
    else taps<UP, LO, 3>(ku, kl, 4 * c, w, acc);
}

__global__ __launch_bounds__(NT) void filter2d_kernel(const float* __restrict__ x, const float* __restrict__ kern, float* __restrict__ y,
                                                      BlurGeom m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* tk = reinterpret_cast<double*>(smem);
    float* t = reinterpret_cast<float*>(smem + m.tap_bytes);
    const int K = m.K, r = K >> 1, KK = K * K, pitch = m.pitch;
    const int pl = blockIdx.x / m.tiles, tile = blockIdx.x - pl * m.tiles;
    const int ty0 = tile / m.gx, tx0 = tile - ty0 * m.gx;
    const int y0 = ty0 * TH, x0 = tx0 * TW;
    const int64_t plane = (int64_t)m.H * m.W;
    const float* xp = x + (int64_t)pl * plane;
    float* yp = y + (int64_t)pl * plane;
    const float* kp = kern + (m.per_image ? (int64_t)(pl / m.C) * KK : 0);

    for (int i = threadIdx.x; i < KK; i += NT) tk[i] = (double)kp[i];
    const int LH = TH + K - 1, LW = TW + K - 1;
    for (int ly = threadIdx.x >> 6; ly < LH; ly += NT / 64) {
        const int64_t rb = (int64_t)reflect(y0 + ly - r, m.H) * m.W;
        for (int lx = threadIdx.x & 63; lx < pitch; lx += 64)   // the columns past LW are read by the last 16-byte words and never used
            t[ly * pitch + lx] = lx < LW ? xp[rb + reflect(x0 + lx - r, m.W)] : 0.0f;
    }
    __syncthreads();

    const int c0 = (threadIdx.x & (LANES_X - 1)) * PX, r0 = (threadIdx.x / LANES_X) * PY;
    if (y0 + r0 >= m.H || x0 + c0 >= m.W) return;   // (after the only barrier)
    double acc[PY][PX] = {};
    const float* row = t + r0 * pitch + c0;
    tile_row<true, false>(row, tk, tk, K, acc);
    for (int tt = 1; tt < K; ++tt) tile_row<true, true>(row + tt * pitch, tk + tt * K, tk + (tt - 1) * K, K, acc);
    tile_row<false, true>(row + K * pitch, tk, tk + (K - 1) * K, K, acc);

#pragma unroll
    for (int i = 0; i < PY; ++i) {
        const int rr = y0 + r0 + i;
        if (rr >= m.H) break;
        float* o = yp + (int64_t)rr * m.W + x0 + c0;
        if (x0 + c0 + PX <= m.W && ((uintptr_t)o & 15) == 0) {
            *reinterpret_cast<float4*>(o) = make_float4((float)acc[i][0], (float)acc[i][1], (float)acc[i][2], (float)acc[i][3]);
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j)
                if (x0 + c0 + j < m.W) o[j] = (float)acc[i][j];
        }
    }
}
}  // namespace

int launch_filter2d_fwd(const float* x, const float* kern, float* y, int B, int C, int H, int W, int K, int per_image, hipStream_t s) {
    BlurGeom m{};
    m.C = C; m.H = H; m.W = W; m.K = K;
    m.per_image = per_image;
    m.gx = cdiv(W, TW);
    m.tiles = m.gx * cdiv(H, TH);
    const int64_t blocks = (int64_t)m.tiles * B * C;   // (the entry point keeps it below 2^31)
    // the last 16-byte word a lane reads starts at column 60 + 4 ceil(K / 4); a pitch that is a multiple of 32 dwords keeps the reads
    // of a wave's four lane rows on disjoint banks
    m.pitch = (TW + 4 * cdiv(K, 4) + 4 + 31) / 32 * 32;
    m.tap_bytes = (K * K * (int)sizeof(double) + 15) / 16 * 16;
    const size_t lds = (size_t)m.tap_bytes + (size_t)(TH + K - 1) * m.pitch * sizeof(float);   // K = 51: 20816 + 41984 = 62800 bytes
    trace_tag("degrade.filter2d");
    filter2d_kernel<<<dim3((unsigned)blocks), dim3(NT), lds, s>>>(x, kern, y, m);
    DCPT_CHECK_LAUNCH("filter2d_fwd");
    return DCPT_OK;
}
