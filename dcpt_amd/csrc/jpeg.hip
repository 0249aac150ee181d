// The JPEG round trip of DiffJPEG on the device (include/dcpt_hip.h dcpt_diffjpeg_fwd): the reference's DiffJPEG.forward
// (basicsr/utils/diffjpeg.py:494-523) in ONE launch, one read of the image and one write.  x, y: fp32 NCHW [B][C][H][W] in [0, 1], C = 1 or 3;
// quality: [B] fp32 on the device, one value per image.  Stage by stage, on one 16 x 16 macroblock (4 Y blocks + Cb + Cr of 8 x 8):
//     zero padding of the bottom / right edge to a multiple of 16 (:509-515): by addressing, a pixel outside the plane reads as 0
//     v = 255 x (:256);  with DCPT_JPEG_UINT8_IO v = rint(255 x): the 8-bit image cv2.imencode is given at paired_image_dataset.py:539
//     Y = .299 R + .587 G + .114 B,  Cb = -.168736 R - .331264 G + .5 B + 128,  Cr = .5 R - .418688 G - .081312 B + 128 (:59-85)
//     Cb, Cr: the mean of each 2 x 2 quad (:88-119)
//     F[u][v] = a(u) a(v) / 4 * sum_xy (s[x][y] - 128) cos((2x + 1) u pi / 16) cos((2y + 1) v pi / 16), a(0) = 1 / sqrt 2, a(k > 0) = 1 (:144-171)
//     t = F[u][v] / (table[u][v] * factor), table the TRANSPOSED luma table for Y (:15-28) and the chroma table (:29-34), factor =
//         quality_to_factor(quality[b]) (:42-55): 50 / q below 50, 2 - q / 50 from 50 on
//     r = rint(t), half to even as torch.round;  with DCPT_JPEG_DIFF_ROUND r = rint(t) + (t - rint(t))^3 (:37-39)
//     D = r * (table * factor) (:273-318);  s'[u][v] = 1/4 sum_xy a(x) a(y) D[x][y] cos((2u + 1) x pi / 16) cos((2v + 1) y pi / 16) + 128 (:321-346)
//     chroma repeated 2 x 2 (:372-398);  R = Y + 1.402 (Cr - 128), G = Y - .344136 (Cb - 128) - .714136 (Cr - 128), B = Y + 1.772 (Cb - 128)
//     (:401-423);  clamp to [0, 255], / 255 (:467-470);  crop to H x W (:519): by predication, nothing is written for the pad
//     C == 1: the plane is all three channels (:507-508), the output the mean of the three decoded channels (:521-522)
//     DCPT_JPEG_UINT8_IO: the output is rint(clamped) / 255, what cv2.imdecode followed by / 255 gives (paired_image_dataset.py:544-546);
//     with C == 1 it is rint(mean of the three clamped channels) / 255
//
// Everything is fp64, from the pixel load to the single rounding to fp32 at the store: the rounding decision rint(t) never hinges on an
// fp32 summation order.  The one departure from the reference: its fp32 pipeline can round a coefficient the other way when the exact t
// lies within about 1e-4 of a tie.
//
// One wave per macroblock, four horizontally adjacent macroblocks per workgroup of 256.  A lane owns one 2 x 2 pixel quad (so the chroma
// mean needs no other lane) and, in the transforms, element (lane / 8, lane % 8) of each of the six blocks.  The 384 samples of the
// macroblock sit in LDS in fp64 (two buffers of 3 KB per wave: a pass reads one and writes the other); each DCT / iDCT is two separable
// 8-point passes with the lane's 8 cosines in registers.  No workspace, no atomics, no global state; an image's result depends on its own
// pixels and its own quality alone, and is the same bits on every run.
#include <math.h>

#include "kernels.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {
constexpr int NT = 256, WAVES = NT / 64;   // macroblocks per workgroup
constexpr int MB = 16;                     // macroblock edge
constexpr int NS = 384;                    // samples per macroblock: 4 x 64 Y, 64 Cb, 64 Cr

struct JpegGeom {
    int C, H, W;
    int gx;      // workgroups per row of macroblocks
    int flags;
};

__device__ const double kCos16[9] = {1.0, 0.98078528040323045, 0.92387953251128676, 0.83146961230254524, 0.70710678118654752,
                                     0.55557023301960222, 0.38268343236508977, 0.19509032201612827, 0.0};   // cos(k pi / 16), k = 0..8
// the luma table as the JPEG standard prints it (diffjpeg.py:16-25 before its .T); the coefficient (u, v) is divided by kLuma[v][u]
__device__ const unsigned char kLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                            14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                            18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
__device__ const unsigned char kChroma[16] = {17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 99, 47, 66, 99, 99};   // symmetric; 99 elsewhere

__device__ __forceinline__ double cos16(int k) {   // cos(k pi / 16) for any k >= 0, from the first quadrant
    k &= 31;
    if (k > 16) k = 32 - k;
    const bool neg = k > 8;
    if (neg) k = 16 - k;
    const double v = kCos16[k];
    return neg ? -v : v;
}

__device__ __forceinline__ double clamp255(double v) { return fmin(255.0, fmax(0.0, v)); }

__global__ __launch_bounds__(NT) void diffjpeg_kernel(const float* __restrict__ x, const float* __restrict__ quality, float* __restrict__ y,
                                                      JpegGeom m) {
    __shared__ double sa[WAVES][NS], sb[WAVES][NS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int by = blockIdx.x / m.gx, bx = blockIdx.x - by * m.gx;
    const int img = blockIdx.y;
    const int y0 = by * MB, x0 = (bx * WAVES + wave) * MB;   // (x0 may lie past the plane in the row's last workgroup: all pad, no store)
    double* A = sa[wave];
    double* T = sb[wave];
    const int64_t plane = (int64_t)m.H * m.W;
    const int64_t base = (int64_t)img * m.C * plane;
    const bool u8 = (m.flags & 2) != 0, dround = (m.flags & 1) != 0;
    const int qy = lane >> 3, qx = lane & 7;   // the lane's 2 x 2 quad

    // ---- load, x 255, RGB -> YCbCr, chroma mean: samples minus 128 into A ----
    {
        double cbs = 0.0, crs = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ry = 2 * qy + (k >> 1), rx = 2 * qx + (k & 1);
            const int py = y0 + ry, px = x0 + rx;
            double r = 0.0, g = 0.0, b = 0.0;
            if (py < m.H && px < m.W) {
                const int64_t off = base + (int64_t)py * m.W + px;
                r = (double)x[off];
                if (m.C == 3) {
                    g = (double)x[off + plane];
                    b = (double)x[off + 2 * plane];
                } else {
                    g = r;
                    b = r;
                }
            }
            r *= 255.0; g *= 255.0; b *= 255.0;
            if (u8) {
                r = rint(r); g = rint(g); b = rint(b);
            }
            const double Y = 0.299 * r + 0.587 * g + 0.114 * b;
            cbs += -0.168736 * r - 0.331264 * g + 0.5 * b + 128.0;
            crs += 0.5 * r - 0.418688 * g - 0.081312 * b + 128.0;
            A[((ry >> 3) * 2 + (rx >> 3)) * 64 + (ry & 7) * 8 + (rx & 7)] = Y - 128.0;
        }
        A[256 + lane] = cbs * 0.25 - 128.0;
        A[320 + lane] = crs * 0.25 - 128.0;
    }
    __syncthreads();

    const int i = lane >> 3, j = lane & 7;   // the lane's element of every 8 x 8 block
    const double inv_sqrt2 = 0.70710678118654752;
    // ---- DCT, columns of the block first: T[x][v] = sum_y A[x][y] cos((2y + 1) v pi / 16), here x = i, v = j ----
    {
        double c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = cos16((2 * k + 1) * j);
#pragma unroll
        for (int blk = 0; blk < 6; ++blk) {
            const double* row = A + blk * 64 + i * 8;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fma(row[k], c[k], acc);
            T[blk * 64 + lane] = acc;
        }
    }
    __syncthreads();
    // ---- F[u][v] = a(u) a(v) / 4 sum_x T[x][v] cos((2x + 1) u pi / 16), here u = i, v = j; quantise, round, dequantise into A ----
    {
        double c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = cos16((2 * k + 1) * i);
        const double scale = (i == 0 ? inv_sqrt2 : 1.0) * (j == 0 ? inv_sqrt2 : 1.0) * 0.25;
        const double q = (double)quality[img];
        const double factor = (q < 50.0 ? 5000.0 / q : 200.0 - q * 2.0) / 100.0;
        const double dluma = (double)kLuma[j * 8 + i] * factor;
        const double dchroma = (double)((i < 4 && j < 4) ? kChroma[i * 4 + j] : (unsigned char)99) * factor;
#pragma unroll
        for (int blk = 0; blk < 6; ++blk) {
            const double* col = T + blk * 64 + j;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fma(col[k * 8], c[k], acc);
            const double div = blk < 4 ? dluma : dchroma;
            const double t = scale * acc / div;
            double r = rint(t);
            if (dround) {
                const double d = t - r;
                r = r + d * d * d;
            }
            A[blk * 64 + lane] = r * div;
        }
    }
    __syncthreads();
    // ---- iDCT: T[x][v] = sum_y a(y) D[x][y] cos((2v + 1) y pi / 16), here x = i (a frequency), v = j (a position) ----
    {
        double c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = cos16((2 * j + 1) * k);
        c[0] = inv_sqrt2;
#pragma unroll
        for (int blk = 0; blk < 6; ++blk) {
            const double* row = A + blk * 64 + i * 8;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fma(row[k], c[k], acc);
            T[blk * 64 + lane] = acc;
        }
    }
    __syncthreads();
    // ---- s'[u][v] = 1/4 sum_x a(x) T[x][v] cos((2u + 1) x pi / 16) + 128, here u = i, v = j ----
    {
        double c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = cos16((2 * i + 1) * k);
        c[0] = inv_sqrt2;
#pragma unroll
        for (int blk = 0; blk < 6; ++blk) {
            const double* col = T + blk * 64 + j;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fma(col[k * 8], c[k], acc);
            A[blk * 64 + lane] = 0.25 * acc + 128.0;
        }
    }
    __syncthreads();
    // ---- chroma repeat, YCbCr -> RGB, clamp, / 255, store the pixels of the plane ----
    {
        const double cb = A[256 + lane] - 128.0, cr = A[320 + lane] - 128.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ry = 2 * qy + (k >> 1), rx = 2 * qx + (k & 1);
            const int py = y0 + ry, px = x0 + rx;
            if (py >= m.H || px >= m.W) continue;
            const double Y = A[((ry >> 3) * 2 + (rx >> 3)) * 64 + (ry & 7) * 8 + (rx & 7)];
            const double r = clamp255(Y + 1.402 * cr);
            const double g = clamp255(Y - 0.344136 * cb - 0.714136 * cr);
            const double b = clamp255(Y + 1.772 * cb);
            const int64_t off = base + (int64_t)py * m.W + px;
            if (m.C == 3) {
                y[off] = (float)((u8 ? rint(r) : r) / 255.0);
                y[off + plane] = (float)((u8 ? rint(g) : g) / 255.0);
                y[off + 2 * plane] = (float)((u8 ? rint(b) : b) / 255.0);
            } else {
                y[off] = u8 ? (float)(rint((r + g + b) / 3.0) / 255.0) : (float)((r / 255.0 + g / 255.0 + b / 255.0) / 3.0);
            }
        }
    }
}
}  // namespace

int launch_diffjpeg_fwd(const float* x, const float* quality, float* y, int B, int C, int H, int W, int flags, hipStream_t s) {
    JpegGeom m{};
    m.C = C; m.H = H; m.W = W;
    m.gx = cdiv(cdiv(W, MB), WAVES);
    m.flags = flags;
    trace_tag("jpeg.fwd");
    diffjpeg_kernel<<<dim3((unsigned)(m.gx * cdiv(H, MB)), (unsigned)B), dim3(NT), 0, s>>>(x, quality, y, m);
    DCPT_CHECK_LAUNCH("diffjpeg_fwd");
    return DCPT_OK;
}
