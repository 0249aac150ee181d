// On-the-fly degradations of the demosaic and inpainting data paths (include/dcpt_hip.h dcpt_demosaic_fwd, dcpt_inpaint_lines_fwd): lq from
// gt in ONE launch each, one read of the batch and one write, no workspace, no atomics, the same bits on every run.
//
// ---- dcpt_demosaic_fwd ----
// x: fp32 NCHW [B][C][H][W], C = 3 (an RGB image: the Bayer mosaic is taken while loading) or C = 1 (the CFA plane itself); y: [B][3][H][W].
// The CFA sample at (r, c) is R where r and c are even, B where both are odd, G otherwise (RGGB, masks_CFA_Bayer of the reference's
// basicsr/utils/mosaic_util.py).  Default: Malvar-He-Cutler (dm_matlab there), 5 x 5, the CFA plane reflect-padded by 2 (-1 -> 1, -2 -> 2,
// H -> H - 2, H + 1 -> H - 3; the reflection keeps the parity, so it keeps the colour).  In units of 1/16, c the centre, h1 / v1 the sums of
// the two horizontal / vertical neighbours at distance 1, h2 / v2 at distance 2, d the sum of the four diagonal neighbours:
//     kgrb   G at an R or B site                                  8 c + 4 (h1 + v1) - 2 (h2 + v2)
//     krbg0  R at (even, odd), B at (odd, even)                  10 c + 8 h1 - 2 h2 + v2 - 2 d
//     krbg0' R at (odd, even), B at (even, odd)                  10 c + 8 v1 - 2 v2 + h2 - 2 d
//     krbbr  R at a B site, B at an R site                       12 c + 4 d - 3 (h2 + v2)
// and the known sample passes through.  DCPT_DEMOSAIC_BILINEAR: dm there, 3 x 3 on the three sparse colour planes with CIRCULAR padding; in
// units of 1/4, R and B weigh a neighbour (2 - |dy|) (2 - |dx|), G weighs the centre 4 and the four axis neighbours 1, and a neighbour
// counts for the colour of the position it wraps to (with an odd H or W the parity, hence the colour, changes across the seam).
// Arithmetic: fp32 sums of the raw x scaled by 1/16 (1/4), no clamp and no rounding -- or, with DCPT_DEMOSAIC_UINT8_IO, integers:
// v = rint(clamp(x, 0, 1) * 255) (the product in fp32), S = sum tap * v, y = float(rint(clamp(S / 16, 0, 255))) / 255.0f, rint half to even.
// Odd H and W are an extension: the reference's mosaic_CFA_Bayer refuses them.
//
// A bandwidth kernel: one 16 x 64 output tile per workgroup of 256; the CFA tile with its 2-pixel halo (20 x 68 words, 5.4 KB) is staged
// once in LDS, picked by parity from the RGB planes while loading, lanes along W for the loads, the LDS reads (stride-1: no bank conflict)
// and the three stores; the image index is the grid's y.
//
// ---- dcpt_inpaint_lines_fwd ----
// x, y: fp32 [B][C][H][W], C = 1 or 3, in place allowed (a pixel is read and written by one lane).  lines: int32 [B][10][4] = x1, y1, x2, y2;
// meta: int32 [B][3] = n_lines, thick, white.  A pixel p is masked when it lies within thick / 2 of one of the first n_lines segments, in
// exact int64 arithmetic with q = p - P1, d = P2 - P1, a = q . d, L = d . d:
//     a <= 0: 4 |q|^2 <= thick^2 (covers L = 0);   a >= L: 4 |q - d|^2 <= thick^2;   otherwise 4 (q x d)^2 <= thick^2 L
// A masked pixel becomes 1 (white) or 0 in every channel, any other clamp(x, 0, 1): np.clip(img +- mask, 0, 1) of the reference's
// PairedImageInpaintingDataset.inpainting.  Values the entry point cannot see without a synchronisation are clamped here: n_lines to 0..10,
// thick to 1..64, an endpoint coordinate to -16384..16384 (with H, W <= 16384 the triangle p, P1, P2 lies in a square of side 32768, so
// |q x d| <= 2^30 and 4 (q x d)^2 <= 2^62).
#include <math.h>

#include "kernels.h"
#include "prof.h"

namespace {
constexpr int NT = 256;
constexpr int TW = 64, TH = 16;            // the output tile
constexpr int HALO = 2;
constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
constexpr int ROWS = TH / (NT / TW);       // rows of the tile per lane
constexpr int MAX_LINES = 10;

struct MosaicGeom {
    int C, H, W;
    int gx;      // tiles per row of tiles
};

// the padded coordinate i in -2 .. n + 1 brought into the plane; anything farther out (the halo of a ragged tile: never used) is clamped
template <bool BILIN>
__device__ __forceinline__ int wrap(int i, int n) {
    if (BILIN) i = i < 0 ? i + n : (i >= n ? i - n : i);
    else i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return min(max(i, 0), n - 1);
}

template <bool U8>
__device__ __forceinline__ float finish(float s, float scale) {   // s: the sum in units of 1 / 16 or 1 / 4 (an exact integer under U8)
    const float v = s * scale;
    if (!U8) return v;
    return rintf(fminf(fmaxf(v, 0.0f), 255.0f)) / 255.0f;
}

template <bool U8, bool BILIN>
__global__ __launch_bounds__(NT) void demosaic_kernel(const float* __restrict__ x, float* __restrict__ y, MosaicGeom m) {
    // fp32 holds the 8-bit samples and every tap sum of them exactly (|S| <= 40 * 255), so one LDS image serves both arithmetics
    __shared__ float t[LH * LW];
    const int ty0 = blockIdx.x / m.gx, tx0 = blockIdx.x - ty0 * m.gx;
    const int y0 = ty0 * TH, x0 = tx0 * TW;
    const int64_t plane = (int64_t)m.H * m.W;
    const float* xb = x + (int64_t)blockIdx.y * m.C * plane;
    float* yb = y + (int64_t)blockIdx.y * 3 * plane;

    for (int i = threadIdx.x; i < LH * LW; i += NT) {
        const int ly = i / LW, lx = i - ly * LW;
        const int r = wrap<BILIN>(y0 + ly - HALO, m.H), c = wrap<BILIN>(x0 + lx - HALO, m.W);
        int ch = 0;
        if (m.C == 3) ch = (r & 1) == (c & 1) ? (r & 1) * 2 : 1;
        float v = xb[ch * plane + (int64_t)r * m.W + c];
        if (U8) v = rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
        t[i] = v;
    }
    __syncthreads();

    const int lx = threadIdx.x & (TW - 1), lyb = (threadIdx.x / TW) * ROWS;
    const int c = x0 + lx;
    if (c >= m.W) return;
    int cpar[3];   // bilinear: the colour parity of the columns c - 1, c, c + 1 where they wrap to
#pragma unroll
    for (int k = 0; k < 3; ++k) cpar[k] = wrap<true>(c + k - 1, m.W) & 1;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int ly = lyb + k, r = y0 + ly;
        if (r >= m.H) break;
        const float* p = t + (ly + HALO) * LW + lx + HALO;
        float R, G, Bl;
        if (BILIN) {
            float sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int rp = wrap<true>(r + dy, m.H) & 1;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int cp = cpar[dx + 1];
                    const float v = p[dy * LW + dx];
                    const float wrb = (float)((2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx)));
                    const float wg = (dy == 0 && dx == 0) ? 4.0f : ((dy == 0 || dx == 0) ? 1.0f : 0.0f);
                    if (rp != cp) sg += wg * v;
                    else if (rp == 0) sr += wrb * v;
                    else sb += wrb * v;
                }
            }
            R = finish<U8>(sr, 0.25f);
            G = finish<U8>(sg, 0.25f);
            Bl = finish<U8>(sb, 0.25f);
        } else {
            const float ctr = p[0];
            const float h1 = p[-1] + p[1], v1 = p[-LW] + p[LW];
            const float h2 = p[-2] + p[2], v2 = p[-2 * LW] + p[2 * LW];
            const float d = (p[-LW - 1] + p[-LW + 1]) + (p[LW - 1] + p[LW + 1]);
            const float known = U8 ? ctr / 255.0f : ctr;   // the sample the CFA holds passes through
            const int rp = r & 1, cp = c & 1;
            if (rp == cp) {
                const float g = finish<U8>(8.0f * ctr + 4.0f * (h1 + v1) - 2.0f * (h2 + v2), 0.0625f);
                const float o = finish<U8>(12.0f * ctr + 4.0f * d - 3.0f * (h2 + v2), 0.0625f);
                G = g;
                R = rp ? o : known;
                Bl = rp ? known : o;
            } else {
                const float hz = finish<U8>(10.0f * ctr + 8.0f * h1 - 2.0f * h2 + v2 - 2.0f * d, 0.0625f);
                const float vt = finish<U8>(10.0f * ctr + 8.0f * v1 - 2.0f * v2 + h2 - 2.0f * d, 0.0625f);
                G = known;
                R = rp ? vt : hz;
                Bl = rp ? hz : vt;
            }
        }
        const int64_t off = (int64_t)r * m.W + c;
        yb[off] = R;
        yb[off + plane] = G;
        yb[off + 2 * plane] = Bl;
    }
}

struct InpaintGeom {
    int C, H, W;
};

__global__ __launch_bounds__(NT) void inpaint_lines_kernel(const float* x, const int* __restrict__ lines, const int* __restrict__ meta, float* y,
                                                           InpaintGeom m) {
    __shared__ int sl[MAX_LINES * 4];
    const int img = blockIdx.z;
    if (threadIdx.x < MAX_LINES * 4) sl[threadIdx.x] = min(max(lines[(int64_t)img * MAX_LINES * 4 + threadIdx.x], -16384), 16384);
    const int n = min(max(meta[img * 3 + 0], 0), MAX_LINES);
    const int64_t thick = min(max(meta[img * 3 + 1], 1), 64);
    const float fill = meta[img * 3 + 2] ? 1.0f : 0.0f;
    __syncthreads();
    const int px = blockIdx.x * TW + (threadIdx.x & (TW - 1)), py = blockIdx.y * (NT / TW) + threadIdx.x / TW;
    if (px >= m.W || py >= m.H) return;
    const int64_t t2 = thick * thick;
    bool masked = false;
    for (int k = 0; k < n; ++k) {
        const int64_t qx = px - sl[4 * k], qy = py - sl[4 * k + 1];
        const int64_t dx = sl[4 * k + 2] - sl[4 * k], dy = sl[4 * k + 3] - sl[4 * k + 1];
        const int64_t a = qx * dx + qy * dy, L = dx * dx + dy * dy;
        bool in;
        if (a <= 0) {
            in = 4 * (qx * qx + qy * qy) <= t2;
        } else if (a >= L) {
            const int64_t ex = qx - dx, ey = qy - dy;
            in = 4 * (ex * ex + ey * ey) <= t2;
        } else {
            const int64_t cr = qx * dy - qy * dx;
            in = 4 * cr * cr <= t2 * L;
        }
        masked = masked || in;
    }
    const int64_t plane = (int64_t)m.H * m.W;
    const int64_t off = (int64_t)img * m.C * plane + (int64_t)py * m.W + px;
    for (int ch = 0; ch < m.C; ++ch) {
        const float v = x[off + ch * plane];
        y[off + ch * plane] = masked ? fill : fminf(fmaxf(v, 0.0f), 1.0f);
    }
}
}  // namespace

int launch_demosaic_fwd(const float* x, float* y, int B, int C, int H, int W, int flags, hipStream_t s) {
    MosaicGeom m{};
    m.C = C; m.H = H; m.W = W;
    m.gx = cdiv(W, TW);
    const dim3 grid((unsigned)((int64_t)m.gx * cdiv(H, TH)), (unsigned)B), block(NT);
    const bool bilin = (flags & 1) != 0, u8 = (flags & 2) != 0;
    trace_tag("degrade.demosaic");
    if (u8 && bilin) demosaic_kernel<true, true><<<grid, block, 0, s>>>(x, y, m);
    else if (u8) demosaic_kernel<true, false><<<grid, block, 0, s>>>(x, y, m);
    else if (bilin) demosaic_kernel<false, true><<<grid, block, 0, s>>>(x, y, m);
    else demosaic_kernel<false, false><<<grid, block, 0, s>>>(x, y, m);
    DCPT_CHECK_LAUNCH("demosaic_fwd");
    return DCPT_OK;
}

int launch_inpaint_lines_fwd(const float* x, const int* lines, const int* meta, float* y, int B, int C, int H, int W, hipStream_t s) {
    InpaintGeom m{};
    m.C = C; m.H = H; m.W = W;
    trace_tag("degrade.inpaint_lines");
    inpaint_lines_kernel<<<dim3((unsigned)cdiv(W, TW), (unsigned)cdiv(H, NT / TW), (unsigned)B), dim3(NT), 0, s>>>(x, lines, meta, y, m);
    DCPT_CHECK_LAUNCH("inpaint_lines_fwd");
    return DCPT_OK;
}
