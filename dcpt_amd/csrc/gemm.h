// fp32 MFMA GEMM family for NHWC activations (rows = pixels, columns = channels).
//
//   NT : C[m][n]  = sum_k A'(m,k) * Bw[n][k]        (1x1-conv forward; dgrad with Bw = W^T)
//   TN : G[n][k]  = sum_m X'(m,n) * Y'(m,k)          (wgrad, split over m into slabs)
//
// Both run on v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD = the fp32 peak of gfx950).
// A'/X'/Y' are produced by fused operand loaders, C is consumed by fused epilogues.
#pragma once
#include "dcpt_common.h"

enum GemmALoad { A_PLAIN = 0, A_LN = 1, A_SCALE = 2, A_SG = 3, A_GATHER = 4, A_CONV3 = 5, A_LNBF = 6, A_CONV3UP = 7 };
enum GemmEpi { E_PLAIN = 0, E_BIAS = 1, E_RESID = 2, E_SGBWD = 3, E_SCATTER = 4, E_SCATTER_ADD = 5, E_ADDSCALED = 6, E_MUL = 7, E_BIASGATE = 8, E_DOTCOL = 9, E_LNBWD = 10, E_RESIDLN = 11, E_RELU = 13, E_BIASCOL = 14, E_PSHUF = 15, E_LRELU = 16 };

struct GemmNT {
    const float* A;   // [M][lda]   (A_SG: 2K columns; A_GATHER: fine NHWC image, see g*)
    const float* Bw;  // [N][K] row-major (K contiguous)
    float* C;         // [M][ldc]   (E_SGBWD: 2N columns; E_SCATTER*: fine NHWC image)
    int64_t M;
    int N, K;
    int lda, ldc;
    // A_LN: a = (x - mu[m]) * rstd[m] * lnw[k] + lnb[k];   A_LNBF (Restormer BiasFree): a = x * rstd[m] * lnw[k]
    const float* mu;
    const float* rstd;
    const float* lnw;
    const float* lnb;
    // A_SCALE: a = x * simg[(m / P) * K + k]   (P = pixels per image)
    const float* simg;
    int P;
    // A_GATHER / E_SCATTER*: coarse grid gH x gW per image, fine image is 2gH x 2gW with gC channels;
    // column index = (2*i + j) * gC + ch  <->  fine pixel (2h+i, 2w+j), channel ch
    // A_CONV3 (implicit GEMM of a dense 3x3, zero pad 1): image gH x gW with gC channels, K = 9*gC,
    // column index = tap * gC + ch, tap = 3*ky + kx  <->  pixel (h+ky-1, w+kx-1)
    // A_CONV3UP: the same 3x3 over the nearest-neighbour 2x up-sampling of a gH x gW image, which is never materialised: the rows are
    // the pixels of the 2gH x 2gW grid (M = B*2gH*2gW), tap pixel (h', w') of that grid (zero padding applied there) reads source
    // pixel (h' >> 1, w' >> 1)
    int gH, gW, gC;
    // epilogues
    const float* bias;    // [N] (may be null)
    const float* res;     // E_RESID / E_ADDSCALED: [M][ldres]; E_SCATTER_ADD: fine image like C
    const float* cscale;  // E_RESID: C = res + (acc+bias)*cscale[n] (null = 1); E_ADDSCALED: C = acc + cscale[n]*res
                          // E_MUL: C = (acc+bias)*res
    const float* aux;     // E_SGBWD: v [M][2N]
    // E_LNBWD (N <= 128, one tile spans the row): the accumulator row g is the gradient of a LayerNorm output whose input was
    // res (x); C = rstd*(g*lnw - mean_c(g*lnw) - xhat*mean_c(g*lnw*xhat)) + aux (the residual gradient, may be null), and
    // colpart[m / 128][0][n] = sum_rows g*xhat (-> dweight), colpart[m / 128][1][n] = sum_rows g (-> dbias); uses mu, rstd, lnw
    // E_RESIDLN (N <= 128): C as E_RESID AND the LayerNorm of that output row: ln_out[m][n] = (C - mean) * rstd * lnw[n] + lnb[n],
    // ln_mu[m], ln_rstd[m] (biased variance about the mean, eps inside the sqrt) -- the next LayerNorm's forward pass
    float* ln_out;
    float* ln_mu;
    float* ln_rstd;
    float ln_eps;
    float* colpart;       // E_DOTCOL: C = acc as E_PLAIN AND colpart[m / 128][n] = sum over the tile's 128 rows of acc * res[m][n]
                          // (fixed order; SCA backward's per-image channel sums come out of the producing GEMM)
    float* gate;          // E_BIASGATE (N = 2*Ch, SimpleGate input): C = acc + bias as usual AND gate[m][c] = C[m][c] * C[m][Ch + c],
                          // [M][Ch] row-major; a block's tile then holds BN/2 columns of each half
    int ldres;            // row stride of res (0 = ldc)
    // E_RELU: C = relu(acc + bias); with res (a ReLU output of the same shape) the ReLU backward C = [res > 0] (acc + bias)
    // E_BIASCOL: C = acc + bias AND per-image column sums of C: the tile's rows of image b (P = pixels per image) sum to
    //   colpart[(m0 / 128 + b) * N + n] (tile / image pairs that overlap have distinct m0 / 128 + b); fixed order, no atomics
    // E_PSHUF: C = acc + bias written through PixelShuffle(psr) into the fine NHWC image [B][psr gH][psr gW][gC]: column
    //   (i psr + j) gC + ch <-> fine pixel (psr h + i, psr w + j), channel ch (the caller orders the weight rows to match)
    int psr;
    // E_LRELU: C = lrelu(acc + bias, slope); with res (a LeakyReLU output of the same shape, slope > 0) its backward
    //   C = (res > 0 ? 1 : slope) * (acc + bias)   (res == 0 takes the slope branch, as torch does)
    float slope;
    // batching: grid.y = nb1*nb2 problems; pointer offsets b1*s?1 + b2*s?2 (elements)
    int nb1, nb2;
    int64_t sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2, sS1, sS2;
};

int launch_gemm_nt(const GemmNT& p, int aload, int epi, hipStream_t stream);
// The two common fills; the caller sets the epilogue fields (bias, res, slope, psr, colpart, P, LayerNorm pointers) afterwards.
// Implicit 3x3 conv (A_CONV3) of the NHWC map x [B][H][W][Cin] with the packed weight wp [Cout][9 Cin]  (A_CONV3UP: the caller
// puts M on the fine 2H x 2W grid)
inline GemmNT gemm_nt_conv3(const float* x, int B, int H, int W, int Cin, const float* wp, int Cout, float* out, int ldc) {
    GemmNT g{};
    g.M = (int64_t)B * H * W; g.A = x; g.K = 9 * Cin; g.gH = H; g.gW = W; g.gC = Cin; g.Bw = wp; g.N = Cout; g.C = out; g.ldc = ldc;
    return g;
}
// Linear layer on rows: out[m][n] = sum_k A[m][k] W[n][k]
inline GemmNT gemm_nt_linear(const float* A, int lda, int64_t M, int K, const float* W, int N, float* out, int ldc) {
    GemmNT g{};
    g.M = M; g.A = A; g.lda = lda; g.K = K; g.Bw = W; g.N = N; g.C = out; g.ldc = ldc;
    return g;
}
// opt-in split-operand mode (gemm_x3.hip, dcpt_set_gemm_x3): fp32-class results on the bf16 matrix pipe; launch_gemm_nt routes eligible
// launches there while the mode is on
bool gemm_nt_x3_ok(const GemmNT& p, int aload, int epi);
int launch_gemm_nt_x3(const GemmNT& p, int aload, int epi, hipStream_t stream);

struct GemmTN {
    const float* X;  // [M][ldx]  -> rows of G (n index)
    const float* Y;  // [M][ldy]  -> cols of G (k index)
    float* slab;     // [batch][splits][N][K]
    float* colsum;   // [splits * gemm_tn_tiles_k(N, K)][N] partial column sums of X' (may be null)
    int64_t M;
    int N, K;
    int ldx, ldy;
    int splits;        // number of m-chunks (grid.y)
    int64_t rows_per_split;  // multiple of 32
    // Y loader (GemmALoad kinds)
    const float* mu;
    const float* rstd;
    const float* lnw;
    const float* lnb;
    const float* simg;
    int P;
    int gH, gW, gC;  // gather geometry for whichever operand is gathered
    // batching: grid.y = nb1*nb2 problems; X/Y offsets b1*s?1 + b2*s?2; slab of batch z at z*splits*N*K
    int nb1, nb2;
    int64_t sX1, sX2, sY1, sY2;
};

// xload in {A_PLAIN, A_GATHER}; yload any GemmALoad kind
int launch_gemm_tn(const GemmTN& p, int xload, int yload, hipStream_t stream);
// choose a split count / rows_per_split for a TN problem
void gemm_tn_plan(int64_t M, int N, int K, int* splits, int64_t* rows_per_split);
// same, with every split inside one image of P pixels; false if no such plan is near the occupancy target
bool gemm_tn_plan_images(int64_t M, int N, int K, int P, int* splits, int64_t* rows_per_split);
// number of k-tile columns of the TN grid for this shape (= partial colsum rows per split)
int gemm_tn_tiles_k(int N, int K);
// opt-in split-operand mode for the weight-gradient GEMM (gemm_x3.hip)
bool gemm_tn_x3_plan(int64_t M, int N, int K, int* splits, int64_t* rows_per_split);   // false: not a shape / size for the mode
bool gemm_tn_x3_ok(const GemmTN& p, int xload, int yload);
int launch_gemm_tn_x3(const GemmTN& p, int fp32_tiles_k, hipStream_t stream);
