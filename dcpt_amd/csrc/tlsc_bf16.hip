// TLSC local average pooling on a bf16 NHWC map (reference basicsr/archs/arch_util.py:378-396; the fp32 twin is box_rows_kernel /
// box_cols_kernel in misc.hip): box mean with a k1 x k2 window, the (H-k1+1) x (W-k2+1) result replicate-padded back to H x W with
// left / top pads (W-Wo)/2, (H-Ho)/2 rounded down (an even window sits asymmetrically).  The caller clamps k1 <= H, k2 <= W.
//
// What was chosen: the two separable passes of the fp32 kernels -- fp32 running window sums (add the entering element, subtract the leaving
// one), the divide and the ONE rounding to bf16 at the end of pass 2 -- but cut into chunks along the walked axis so that B = 1 still fills
// the chip:
//   pass 1  thread = (b, h, chunk of output columns, 8 channels): window sum of the chunk's first column (k2 loads), then slides
//   pass 2  thread = (b, chunk of output rows, w, 8 channels): likewise down the rows of the fp32 row sums, divides, rounds, stores
// Accuracy of the sums: every bf16 term is exact in fp32, but the terms of a window span binades, so each fp32 add or subtract rounds: a
// window sum is accurate to about k 2^-24 of the window's sum of |x| (k = k2 resp. k1 terms), and the add-then-subtract slides add one such
// rounding pair per step along a chunk (a chunk restarts from a fresh sum, so the drift is bounded by the chunk length, ~100 slides at 2K).
// Both stay far below the one bf16 rounding of the result (2^-8); the float64 test below bounds them with k1 k2 2^-24 mean|x|.
// Lanes run over the channel vectors first (16-byte bf16 / 32-byte fp32 accesses, a pixel's C channels contiguous), then over chunks
// (pass 1) or columns (pass 2).  A chunk is at least k2/4 columns resp. k1/2 rows long (and 8), so the start-up sum costs at most 4 resp. 2
// extra loads per output; pass 1's are re-reads of the row its neighbours are streaming (L2), pass 2's are rows apart in memory.
// Known weakness of pass 1 at narrow C: a 64-lane wave covers 64 / (C/8) chunks that lie L C 2 bytes apart, so at C = 64 it reads eight
// 128-byte segments per load instead of one 1 KB run, and the start-up sum is k2 serial 16-byte loads per thread (384 against ~105 outputs
// at level 0 of a 2K image).  Lanes over adjacent columns of one chunk would coalesce better there; not built.
// The fused single-pass form with the row sums on chip was NOT built: with windows of a third of the map the halo exceeds any tile that
// fits LDS.  The fp32 row sums go through memory instead, but in a buffer the block owns anyway (nafblock_bf16.hip puts them where t1,
// dead by then, lies: no workspace of their own).
// Bytes moved per output element -- an ESTIMATE from the access pattern, not a counter measurement (Wo/W = 1 - (k2-1)/W of the row-sum
// terms): 2 (map read) + 4 Wo/W (row sums written) + 4 Wo/W (row sums read, once per chunk that needs them: x (1 + k1 / chunk rows) <= 3
// where the re-reads miss the caches) + 2 (mean map written) = 4 + 8 Wo/W ... 4 + 16 Wo/W, against 16 for the fp32 kernels on an fp32
// map.  The start-up re-reads of pass 1 are not in this figure.  Measured times of the kernel pair are in DESIGN.md section 7.
//
// Index arithmetic is pinned on its own through the thin entry point dcpt_box_mean_bf16 (tests/test_gpu_tlsc_bf16.py, against a float64
// unfold mean + replicate pad, at most one bf16 rounding apart).
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
__device__ __forceinline__ void f8_stg(float* p, f8 v) {
    stg4(p, v.lo);
    stg4(p + 4, v.hi);
}
__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ f8 f8_slide(f8 acc, f8 in, f8 out) {   // (acc + entering) - leaving, the fp32 kernels' order
    return f8{f4_sub(f4_add(acc.lo, in.lo), out.lo), f4_sub(f4_add(acc.hi, in.hi), out.hi)};
}

// pass 1: rs[b][h][j][c] = sum_{x=j}^{j+k2-1} in[b][h][x][c], j in [0, Wo);  chunk c covers j in [c L, min((c+1) L, Wo))
__global__ __launch_bounds__(256) void box_rows_bf16_kernel(const bf16_t* __restrict__ in, float* __restrict__ rs, int64_t BH, int W, int C, int k2,
                                                            int L, int nch) {
    const int nv = C / 8, Wo = W - k2 + 1;
    const int64_t total = BH * nch * nv;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int v = (int)(i % nv);
    const int64_t t = i / nv;
    const int c = (int)(t % nch);
    const int64_t bh = t / nch;
    const int j0 = c * L;
    if (j0 >= Wo) return;
    const int j1 = j0 + L < Wo ? j0 + L : Wo;
    const bf16_t* src = in + bh * W * (int64_t)C + 8 * v;   // columns j0 .. j1 - 1 + k2 - 1 <= Wo - 1 + k2 - 1 = W - 1
    float* dst = rs + bh * Wo * (int64_t)C + 8 * v;
    f8 acc = f8_zero();
    for (int x = j0; x < j0 + k2; ++x) acc = f8_add(acc, bf8_ldg(src + (int64_t)x * C));
    f8_stg(dst + (int64_t)j0 * C, acc);
#pragma unroll 4
    for (int j = j0 + 1; j < j1; ++j) {
        acc = f8_slide(acc, bf8_ldg(src + (int64_t)(j + k2 - 1) * C), bf8_ldg(src + (int64_t)(j - 1) * C));
        f8_stg(dst + (int64_t)j * C, acc);
    }
}

// pass 2: out[b][h][w][c] = bf16((sum_{y=r}^{r+k1-1} rs[b][y][cw][c]) / (k1 k2)),  r = clamp(h - pt, 0, Ho - 1),  cw = clamp(w - pl, 0, Wo - 1);
// chunk c covers output rows h in [c LH, min((c+1) LH, H))
__global__ __launch_bounds__(256) void box_cols_bf16_kernel(const float* __restrict__ rs, bf16_t* __restrict__ out, int B, int H, int W, int C, int k1,
                                                            int k2, int LH, int nch) {
    const int nv = C / 8, Wo = W - k2 + 1, Ho = H - k1 + 1;
    const int pl = (W - Wo) / 2, pt = (H - Ho) / 2;
    const int64_t total = (int64_t)B * nch * W * nv;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int v = (int)(i % nv);
    int64_t t = i / nv;
    const int w = (int)(t % W);
    t /= W;
    const int c = (int)(t % nch);
    const int64_t b = t / nch;
    const int h0 = c * LH;
    if (h0 >= H) return;
    const int h1 = h0 + LH < H ? h0 + LH : H;
    int cw = w - pl;
    cw = cw < 0 ? 0 : (cw > Wo - 1 ? Wo - 1 : cw);
    const float* src = rs + (b * H * (int64_t)Wo + cw) * C + 8 * v;   // row y at src + y * rstride, y <= Ho - 1 + k1 - 1 = H - 1
    const int64_t rstride = (int64_t)Wo * C;
    const float den = (float)((int64_t)k1 * k2);
    int r = h0 - pt;
    r = r < 0 ? 0 : (r > Ho - 1 ? Ho - 1 : r);
    f8 acc = f8_zero();
    for (int y = r; y < r + k1; ++y) acc = f8_add(acc, f8_ld(src + y * rstride));
    for (int h = h0; h < h1; ++h) {
        int want = h - pt;
        want = want < 0 ? 0 : (want > Ho - 1 ? Ho - 1 : want);
        if (r < want) {   // (the window start moves by at most one row per output row; r < want <= Ho - 1 keeps r + k1 <= H - 1)
            acc = f8_slide(acc, f8_ld(src + (int64_t)(r + k1) * rstride), f8_ld(src + (int64_t)r * rstride));
            ++r;
        }
        f8 o;
        o.lo = make_float4(acc.lo.x / den, acc.lo.y / den, acc.lo.z / den, acc.lo.w / den);
        o.hi = make_float4(acc.hi.x / den, acc.hi.y / den, acc.hi.z / den, acc.hi.w / den);
        bf8_stg(out + ((b * H + h) * (int64_t)W + w) * C + 8 * v, o);
    }
}

// chunks of the walked axis: enough threads for ~8 waves on each of the 256 CUs, no chunk shorter than lmin outputs
void plan_chunks(int64_t base_threads, int n_out, int lmin, int* len, int* nch) {
    int64_t want = cdiv64((int64_t)256 * 8 * 64, base_threads);
    const int maxch = n_out / lmin;   // (floor: the chunks that result are at least lmin long)
    if (want > maxch) want = maxch;
    if (want < 1) want = 1;
    *len = cdiv(n_out, (int)want);
    *nch = cdiv(n_out, *len);
}

}  // namespace

size_t box_mean_bf16_rowsum_floats(int B, int H, int W, int C, int k2) { return (size_t)B * H * (W - k2 + 1) * C; }

int launch_box_mean_bf16(const bf16_t* in, float* rowsum, bf16_t* out, int B, int H, int W, int C, int k1, int k2, hipStream_t s) {
    DCPT_CHECK_ARG(in && rowsum && out, "box_mean_bf16: null argument");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && k1 >= 1 && k2 >= 1 && k1 <= H && k2 <= W,
                   "box_mean_bf16: bad window %dx%d for %dx%d (C=%d, C %% 8 == 0)", k1, k2, H, W, C);
    trace_tag("tlsc.box_mean_bf16");
    const int nv = C / 8, Wo = W - k2 + 1;
    const double map = (double)B * H * W * C, rsb = (double)B * H * Wo * C * 4.0;
    ProfScope prof(s, PROF_OTHER, (int64_t)B * H * W, C, k1 * k2, 0.0, 4.0 * map + 2.0 * rsb);
    int L, nch, LH, nchh;
    plan_chunks((int64_t)B * H * nv, Wo, k2 / 4 > 8 ? k2 / 4 : 8, &L, &nch);
    plan_chunks((int64_t)B * W * nv, H, k1 / 2 > 8 ? k1 / 2 : 8, &LH, &nchh);
    const int64_t g1 = cdiv64((int64_t)B * H * nch * nv, 256), g2 = cdiv64((int64_t)B * nchh * W * nv, 256);
    DCPT_CHECK_ARG(g1 < (1ll << 31) && g2 < (1ll << 31), "box_mean_bf16: grid too large");
    box_rows_bf16_kernel<<<dim3((unsigned)g1), dim3(256), 0, s>>>(in, rowsum, (int64_t)B * H, W, C, k2, L, nch);
    DCPT_CHECK_LAUNCH("box_rows_bf16");
    box_cols_bf16_kernel<<<dim3((unsigned)g2), dim3(256), 0, s>>>(rowsum, out, B, H, W, C, k1, k2, LH, nchh);
    DCPT_CHECK_LAUNCH("box_cols_bf16");
    return DCPT_OK;
}

extern "C" size_t dcpt_box_mean_bf16_ws_bytes(int B, int H, int W, int C, int k1, int k2) {
    (void)k1;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || k2 < 1) return 0;
    return align_up(box_mean_bf16_rowsum_floats(B, H, W, C, k2 < W ? k2 : W) * sizeof(float), 256);
}

extern "C" int dcpt_box_mean_bf16(const uint16_t* in, uint16_t* out, void* ws, size_t ws_bytes, int B, int H, int W, int C, int k1, int k2,
                                  dcpt_stream_t stream) {
    DCPT_CHECK_ARG(in && out, "box_mean_bf16: null argument");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && k1 >= 1 && k2 >= 1, "box_mean_bf16: bad shape B=%d H=%d W=%d C=%d k=%dx%d", B, H,
                   W, C, k1, k2);
    if (k1 > H) k1 = H;   // arch_util.py:381 k = min(size, kernel)
    if (k2 > W) k2 = W;
    const size_t need = dcpt_box_mean_bf16_ws_bytes(B, H, W, C, k1, k2);
    DCPT_CHECK_WS("box_mean_bf16", ws, ws_bytes, need);
    return launch_box_mean_bf16(in, (float*)ws, out, B, H, W, C, k1, k2, (hipStream_t)stream);
}
