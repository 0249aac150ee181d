/* dcpt_hip.h -- C ABI of libdcpt_hip.so: the MI355X (gfx950) implementation of the DCPT
 * restoration-encoder hot path (NAFNet blocks and the layers between them).
 *
 * Drop-in boundary.  The reference (MILab-PKU/dcpt) has no FFI of its own on this path: its
 * archs call ATen ops from Python (basicsr/archs/nafnet_arch.py) and its only native bindings
 * are the unused JIT extensions under basicsr/ops (layernorm: ops/layernorm/src/layernorm_kernel.cpp
 * :57-60 pybind `forward`/`backward`; fused_act: ops/fused_act/src/fused_bias_act.cpp:14-26).  The
 * entry points below are what a maintainer would bind from the arch modules instead of those ATen
 * calls; each one cites the reference code it replaces.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 data unless it says otherwise; the caller (PyTorch)
 *    owns all buffers, including workspaces and tensors saved for backward;
 *  - feature maps are NHWC ([B][H][W][C], C contiguous; torch `channels_last` memory); only the
 *    network's image input/output is NCHW (3 channels);
 *  - weights keep the reference's state-dict layouts (conv: [out][in][kh][kw]);
 *  - every call enqueues work on `stream` (a hipStream_t) and returns immediately: 0 on success,
 *    non-zero on error (dcpt_last_error() gives the message, per host thread).  No compute call
 *    synchronises with the host or allocates device memory, and none keeps DATA between calls.
 *    Process-wide state that does exist, all of it listed here: (1) two global toggles,
 *    dcpt_set_side_stream() and dcpt_prof_enable() (the latter also owns the event pairs it recorded
 *    until dcpt_prof_read() drains them -- dcpt_prof_read is the one call that waits on the device);
 *    (2) a cache of one internal low-priority HIP stream + 8 events per (device, caller stream),
 *    created on the first backward call that uses it and kept for the life of the process;
 *    (3) the lazily resolved RCCL entry point of dcpt_allreduce_flat().  Calls on different
 *    streams / devices are re-entrant; the toggles are not meant to be flipped concurrently with
 *    launches.
 *  - channel counts must be multiples of 4.
 */
#ifndef DCPT_HIP_H
#define DCPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dcpt_stream_t; /* hipStream_t */

const char* dcpt_last_error(void);
int dcpt_abi_version(void);

/* ---- LayerNorm2d --------------------------------------------------------------------------
 * replaces nafnet_arch.py:25-64 (LayerNormFunction / LayerNorm2d) and ops/layernorm
 * (layernorm_kernel.cpp:14-55).  x,y: [M][C] rows = pixels.  mu/rstd: [M] saved statistics. */
int dcpt_ln2d_fwd(const float* x, const float* weight, const float* bias, float* y, float* mu, float* rstd,
                  int64_t M, int C, float eps, dcpt_stream_t stream);
size_t dcpt_ln2d_bwd_ws_bytes(int64_t M, int C);
int dcpt_ln2d_bwd(const float* dy, const float* x, const float* mu, const float* rstd, const float* weight,
                  float* dx, float* dweight, float* dbias, void* ws, size_t ws_bytes, int64_t M, int C,
                  dcpt_stream_t stream);

/* ---- NAFBlock -----------------------------------------------------------------------------
 * replaces nafnet_arch.py:83-186 (NAFBlock.forward and its autograd backward). */
typedef struct {
    const float* norm1_w; const float* norm1_b;   /* [C] */
    const float* conv1_w; const float* conv1_b;   /* [2C][C][1][1], [2C] */
    const float* conv2_w; const float* conv2_b;   /* [2C][1][3][3], [2C]  (depthwise) */
    const float* conv3_w; const float* conv3_b;   /* [C][C][1][1], [C] */
    const float* sca_w;   const float* sca_b;     /* [C][C][1][1], [C] */
    const float* norm2_w; const float* norm2_b;   /* [C] */
    const float* conv4_w; const float* conv4_b;   /* [2C][C][1][1], [2C] */
    const float* conv5_w; const float* conv5_b;   /* [C][C][1][1], [C] */
    const float* beta;    const float* gamma;     /* [1][C][1][1] */
} dcpt_nafblock_params;

typedef struct {   /* same shapes as dcpt_nafblock_params; all written (not accumulated) */
    float* norm1_w; float* norm1_b;
    float* conv1_w; float* conv1_b;
    float* conv2_w; float* conv2_b;
    float* conv3_w; float* conv3_b;
    float* sca_w;   float* sca_b;
    float* norm2_w; float* norm2_b;
    float* conv4_w; float* conv4_b;
    float* conv5_w; float* conv5_b;
    float* beta;    float* gamma;
} dcpt_nafblock_grads;

typedef struct {   /* activations kept for backward (M = B*H*W pixels) */
    float* t1;      /* [M][2C]  conv1(LN1(inp)) */
    float* t2;      /* [M][C]   SimpleGate(dwconv(t1)) */
    float* y;       /* [M][C]   inp + conv3(t2*s)*beta */
    float* v;       /* [M][2C]  conv4(LN2(y)) */
    float* mu1; float* rstd1; float* mu2; float* rstd2;   /* [M] */
    float* pooled;  /* [B][C]   mean_{h,w} t2 */
    float* s;       /* [B][C]   SCA scale */
    float* xn1;     /* [M][C]   LN1(inp): read back by conv1's forward and weight-gradient GEMMs as a plain operand */
    float* xn2;     /* [M][C]   LN2(y) */
    float* g;       /* [M][C]   SimpleGate(v), written by conv4's GEMM epilogue; conv5's operand in forward and weight gradient */
} dcpt_nafblock_saved;

size_t dcpt_nafblock_fwd_ws_bytes(int B, int H, int W, int C);
size_t dcpt_nafblock_bwd_ws_bytes(int B, int H, int W, int C);
/* inp,out: [B][H][W][C].  `saved` is the forward's scratch for ITS OWN backward (inference callers may recycle the buffers); which of
 * the tensors hold data afterwards is the library's business.  Where dcpt_nafblock_fused_ffn(C) is 1 (C = 64: the forward 1 x 1 chains
 * run as one pass each, ffn_f32.hip) saved->xn1 / xn2 / g are never read or written in either pass and may be NULL (dcpt_nafblock_bwd takes
 * them from its GEMMs' operand loaders), and a caller that will not run the backward pass may also pass v = mu1 = rstd1 = mu2 = rstd2 =
 * NULL: the forward then skips those writes (the second half moves 2 tensor passes instead of 4).  Elsewhere every pointer is required. */
int dcpt_nafblock_fused_ffn(int C);
int dcpt_nafblock_fwd(const dcpt_nafblock_params* p, const float* inp, float* out, const dcpt_nafblock_saved* saved,
                      void* ws, size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream);
/* dout,dinp: [B][H][W][C]; dinp may alias dout. */
int dcpt_nafblock_bwd(const dcpt_nafblock_params* p, const dcpt_nafblock_grads* g, const float* inp,
                      const dcpt_nafblock_saved* saved, const float* dout, float* dinp, void* ws, size_t ws_bytes,
                      int B, int H, int W, int C, dcpt_stream_t stream);

/* ---- Opt-in GEMM precision mode "bf16x3" (gemm_x3.hip): while a scratch buffer is registered, the wide fp32 NT GEMMs of every entry point
 * (plain or per-image-scaled A operand, N % 256 == 0, K % 16 == 0, >= 192 tiles of 256 x 256) run on the bf16 matrix pipe with both operands
 * split into three bfloat16 pieces (x = x0 + x1 + x2 exactly), six piece products per element pair, fp32 accumulation: fp32-CLASS results
 * (not bit-identical to the default fp32-MFMA kernels; the dropped terms are up to 2^-22 of a product, below the fp32 kernel's own error only
 * in a sum of some tens of products, so a weight gradient over fewer than 64 pixels keeps the fp32 kernel).  PROCESS-WIDE state: the scratch (>= 6 bytes per
 * element of the largest A operand + weights) is shared by all launches, which must therefore all be on ONE stream while the mode is on.
 * scratch == NULL switches the mode off (the default).  The reference computes in fp32; this mode is reported separately. */
/* min_tiles: launches with fewer 256 x 256 tiles keep the fp32-MFMA kernels (<= 0: the default, 192 -- most of the 256 CUs busy). */
int dcpt_set_gemm_x3(void* scratch, size_t bytes, int min_tiles);
/* launches since process start that were eligible for the mode but ran on the fp32 kernels because `bytes` was too small for their weight
 * images (a mode that is silently only partly on would be a wrong label on a measurement: callers check this stays 0) */
long long dcpt_gemm_x3_scratch_misses(void);

/* ---- NAFBlock, bf16 storage (BASELINE.json configs[2]) --------------------------------------------------------------
 * Same block (nafnet_arch.py:83-186), activations and saved tensors as bfloat16 (raw uint16_t, upper half of an fp32, stored
 * round-to-nearest-even), fp32 accumulation on v_mfma_f32_32x32x16_bf16, fp32 parameters / parameter gradients / LayerNorm
 * statistics / reductions.  The reference has no reduced-precision mode (its AMP / TF32 switches are commented out,
 * basicsr/test.py:26-27): this is new behaviour with its own tolerance (tests/test_gpu_bf16.py, oracle bf16 mode).
 * C must be a multiple of 8 (16-byte rows), at most 1024.  dinp must NOT alias dout (weight-gradient GEMMs on the side
 * stream still read dout when dinp is written). */
typedef struct {
    uint16_t* t1;   /* [M][2C] bf16 */
    uint16_t* t2;   /* [M][C]  */
    uint16_t* y;    /* [M][C]  */
    uint16_t* v;    /* [M][2C] */
    float* mu1; float* rstd1; float* mu2; float* rstd2;   /* [M] fp32 */
    float* pooled;  /* [B][C] fp32 */
    float* s;       /* [B][C] fp32 */
    uint16_t* xn1;  /* [M][C]  LN1(inp) */
    uint16_t* xn2;  /* [M][C]  LN2(y) */
    uint16_t* g;    /* [M][C]  SimpleGate(v) */
} dcpt_nafblock_saved_bf16;
size_t dcpt_nafblock_fwd_bf16_ws_bytes(int B, int H, int W, int C);
size_t dcpt_nafblock_bwd_bf16_ws_bytes(int B, int H, int W, int C);
/* packed / packed_bytes: the block's dcpt_nafblock_wpack_bf16 buffer (below), or NULL, 0 -- the call then packs the weights into its workspace */
int dcpt_nafblock_fwd_bf16(const dcpt_nafblock_params* p, const void* packed, size_t packed_bytes, const uint16_t* inp, uint16_t* out,
                           const dcpt_nafblock_saved_bf16* saved, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                           dcpt_stream_t stream);
int dcpt_nafblock_bwd_bf16(const dcpt_nafblock_params* p, const void* packed, size_t packed_bytes, const dcpt_nafblock_grads* g,
                           const uint16_t* inp, const dcpt_nafblock_saved_bf16* saved, const uint16_t* dout, uint16_t* dinp, void* ws,
                           size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream);
/* Per-block operand copies of the weights (ABI 7).  Everything the block's GEMMs and depthwise kernels read of the PARAMETERS --
 * bf16 [N][K] copies of conv1 / conv4 / conv5, transposed (beta / gamma-scaled) copies of conv5 / conv4 / conv3 / conv1 for the data
 * gradients, the depthwise taps as [9][2C] fp32 -- depends on the parameters only: a caller that keeps one buffer of
 * dcpt_nafblock_wpack_bf16_bytes(C) per block and re-runs dcpt_nafblock_wpack_bf16 (ONE launch) whenever the block's parameters
 * changed (once per optimizer step) hands it to dcpt_nafblock_fwd/bwd_bf16 as `packed`, which then launch no pack kernels except the
 * per-image SCA-scaled conv3 weights (5 launches fewer per block and step).  Results are bit-identical to those with packed == NULL. */
size_t dcpt_nafblock_wpack_bf16_bytes(int C);
/* 1 when dcpt_nafblock_fwd_bf16 at width C runs the second half of the block (LayerNorm2 -> conv4 -> SimpleGate -> conv5 -> residual,
 * nafnet_arch.py:180-186) as ONE kernel (ffn_bf16.hip, the narrow levels): a caller that will not run the backward pass (inference)
 * may then pass saved->v = xn2 = g = mu2 = rstd2 = NULL -- all five or none -- and the forward skips v as well (4 -> 2 tensor passes for
 * that half).  With 1 the library never reads or writes saved->xn2 / g / mu2 / rstd2 in either pass (its backward kernels recompute
 * LayerNorm2, the gate and the statistics from y and v): in training they only have to be non-null.  0: every saved buffer is used --
 * except that saved->v ALONE may be NULL at any width when no backward pass follows: conv4's bias + gate epilogue then writes
 * SimpleGate(v) only (one tensor pass instead of three for that launch).
 * 2 (ABI 11; C = 256 / 512, chain_bf16.hip: the same chain per 128-pixel tile with the weights streamed past it): the forward WRITES
 * xn2 / g / mu2 / rstd2 (the unfused backward reads them), but a caller that will not run the backward pass may pass all five of
 * v / xn2 / g / mu2 / rstd2 as NULL exactly as with 1. */
int dcpt_nafblock_bf16_fused_ffn(int C);
int dcpt_nafblock_wpack_bf16(const dcpt_nafblock_params* p, void* packed, size_t packed_bytes, int C, dcpt_stream_t stream);
/* The same for n blocks at once (ABI 10; ps / packed / packed_bytes / C are arrays of n, any mix of widths): ceil(n / 8) launches
 * instead of n -- a network's packs once per optimizer step.  Bit-identical to n calls of dcpt_nafblock_wpack_bf16. */
int dcpt_nafblock_wpack_bf16_multi(const dcpt_nafblock_params* ps, void* const* packed, const size_t* packed_bytes, const int* C, int n,
                                   dcpt_stream_t stream);
/* Weight (and bias) gradient of a 1 x 1 convolution in bf16 storage (ABI 9; the conv1 / conv3 / conv4 / conv5 weight gradients of
 * nafnet_arch.py:170-186 as an operator of its own): dW[n][k] = sum_m dY[m][n] * X[m][k], db[n] = sum_m dY[m][n] (db may be NULL).
 * dY: [M][N] bf16, X: [M][K] bf16, dW: [N][K] fp32.  N, K multiples of 8; where both are multiples of 256 the 256 x 256-tile grouped
 * kernel + finisher of gemm_tn_bf16_256.hip run (what dcpt_nafblock_bwd_bf16 uses at the wide levels), else the 128-wide kernel.
 * Deterministic (fixed summation order). */
size_t dcpt_conv1x1_wgrad_bf16_ws_bytes(int64_t M, int N, int K);
int dcpt_conv1x1_wgrad_bf16(const uint16_t* dY, const uint16_t* X, float* dW, float* db, void* ws, size_t ws_bytes, int64_t M, int N, int K,
                            dcpt_stream_t stream);
/* fp32 <-> bf16 (RNE) on n contiguous elements, n % 8 == 0: the edges of the bf16 path */
int dcpt_cast_f32_bf16(const float* x, uint16_t* y, int64_t n, dcpt_stream_t stream);
int dcpt_cast_bf16_f32(const uint16_t* x, float* y, int64_t n, dcpt_stream_t stream);

/* ---- the layers between the NAFBlock groups, bf16 storage (edge_bf16.hip): same algorithms and argument meaning as
 * dcpt_conv3x3_in / _out, dcpt_down2x2 and dcpt_up_ps below (reference basicsr/archs/nafnet_arch.py:202-219, :230, :238-242,
 * :252-272); feature maps (NHWC) and their gradients are bf16, the 3-channel images (NCHW), weights, biases and all parameter
 * gradients fp32.  With these a NAFNet in bf16 storage has no cast kernels between its layers.  down: C % 8 == 0; up: C % 16 == 0.
 * Workspaces: dcpt_conv3x3_in_bwd_ws_bytes / dcpt_conv3x3_out_bwd_ws_bytes (unchanged), dcpt_down2x2_bf16_ws_bytes, dcpt_up_ps_bf16_ws_bytes. */
int dcpt_conv3x3_in_fwd_bf16(const float* x, const float* w, const float* bias, uint16_t* y, int B, int H, int W, int Cin, int Cout,
                             dcpt_stream_t stream);
int dcpt_conv3x3_in_bwd_bf16(const uint16_t* dy, const float* x, const float* w, float* dx /* may be NULL */, float* dw, float* dbias, void* ws,
                             size_t ws_bytes, int B, int H, int W, int Cin, int Cout, dcpt_stream_t stream);
int dcpt_conv3x3_out_fwd_bf16(const uint16_t* x, const float* w, const float* bias, const float* res, float* y, int B, int H, int W, int Cin,
                              int Cout, dcpt_stream_t stream);
int dcpt_conv3x3_out_bwd_bf16(const float* dy, const uint16_t* x, const float* w, uint16_t* dx, float* dw, float* dbias, void* ws, size_t ws_bytes,
                              int B, int H, int W, int Cin, int Cout, dcpt_stream_t stream);
size_t dcpt_down2x2_bf16_ws_bytes(int B, int H, int W, int C, int backward);
int dcpt_down2x2_fwd_bf16(const uint16_t* x, const float* w, const float* bias, uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                          dcpt_stream_t stream);
/* dx = dx_add + the down layer's data gradient (dx_add [B][H][W][C] or NULL): see dcpt_down2x2_bwd */
int dcpt_down2x2_bwd_bf16(const uint16_t* dy, const uint16_t* x, const float* w, const uint16_t* dx_add, uint16_t* dx, float* dw, float* dbias,
                          void* ws, size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream);
size_t dcpt_up_ps_bf16_ws_bytes(int B, int H, int W, int C, int backward);
int dcpt_up_ps_fwd_bf16(const uint16_t* x, const float* w, const uint16_t* skip /* may be NULL */, uint16_t* y, void* ws, size_t ws_bytes, int B,
                        int H, int W, int C, dcpt_stream_t stream);
int dcpt_up_ps_bwd_bf16(const uint16_t* dy, const uint16_t* x, const float* w, uint16_t* dx, float* dw, void* ws, size_t ws_bytes, int B, int H,
                        int W, int C, dcpt_stream_t stream);

/* ---- classifier head, bf16 storage: the conv -> channels-first LayerNorm -> [+shortcut] -> [ReLU] groups and the
 * conv1x1 -> MaxPool2d(2,2) -> ReLU downsamples of degrad_classify_arch.py (:69-103, :227-243, :596-602) with bf16 activations
 * (x, z = conv output, y and their gradients), fp32 parameters / gradients / statistics; same argument meaning as dcpt_conv_ln_* and
 * dcpt_conv1x1_pool_relu_* below.  Channel counts must be multiples of 8, Cout <= 1024. */
/* ABI 14: cached operand copies of the head's conv weights.  With wpacked == NULL the entry points below pack their bf16 operand image of `w`
 * in the call (one small launch in front of each GEMM: 68 per step of the DCPT head).  A caller that keeps one buffer of dcpt_conv_wpack_bf16_bytes(Cin, Cout, ksize) bytes
 * per conv (device memory, 256-byte aligned) fills all of them with dcpt_conv_wpack_bf16_multi (n convs: a launch per 40 convs, the 3 x 3 and the
 * 1 x 1 convs apart) once per optimizer step -- whenever the weights may have changed -- and passes it as `wpacked`: same
 * results bit for bit, no pack launches.  A buffer holds the forward image ([Cout][ksize ksize Cin]) and the data gradient's (transposed; taps
 * flipped for the 3 x 3).  `w` may be NULL only when wpacked is given. */
size_t dcpt_conv_wpack_bf16_bytes(int Cin, int Cout, int ksize);
int dcpt_conv_wpack_bf16_multi(const float* const* w, void* const* packed, const size_t* packed_bytes, const int* Cin, const int* Cout,
                               const int* ksize, int n, dcpt_stream_t stream);
size_t dcpt_conv_ln_bf16_ws_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int backward);
int dcpt_conv_ln_fwd_bf16(const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, const float* lnw, const float* lnb,
                          const uint16_t* res, int relu, uint16_t* z, uint16_t* y, float* mu, float* rstd, void* ws, size_t ws_bytes, int B,
                          int H, int W, int Cin, int Cout, int ksize, dcpt_stream_t stream);
/* dx = dx_add + conv^T(dz) (dx_add [B][H][W][Cin] or NULL; may alias dx).  The BottleneckBlock's input feeds conv1 AND the shortcut
 * (degrad_classify_arch.py:227-243): conv3's dres goes in as conv1's dx_add and the two gradients are summed in the data-gradient GEMM's
 * epilogue instead of by an extra pass over the feature map. */
int dcpt_conv_ln_bwd_bf16(const uint16_t* dy, const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes,
                          const float* lnw, const uint16_t* z, const uint16_t* y, const float* mu, const float* rstd,
                          const uint16_t* dx_add, uint16_t* dx, float* dw, float* dlnw, float* dlnb, uint16_t* dres, void* ws,
                          size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int ksize, int relu, dcpt_stream_t stream);
size_t dcpt_conv1x1_pool_relu_bf16_ws_bytes(int B, int H, int W, int Cin, int Cout, int backward);
int dcpt_conv1x1_pool_relu_fwd_bf16(const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, uint16_t* z, uint16_t* y,
                                    void* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout, dcpt_stream_t stream);
int dcpt_conv1x1_pool_relu_bwd_bf16(const uint16_t* dy, const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes,
                                    const uint16_t* z, uint16_t* dx, float* dw, void* ws, size_t ws_bytes, int B, int H, int W, int Cin,
                                    int Cout, dcpt_stream_t stream);

/* ABI 15: the classifier head's BottleneckBlock as ONE call (reference basicsr/archs/degrad_classify_arch.py:132-243 as the DCPT head builds it:
 * identity shortcut, LN norm, bias-free convs -- relu(LN(conv1 1x1 C -> 2C)) -> relu(LN(conv2 3x3 2C -> 2C)) -> relu(LN(conv3 1x1 2C -> C) + x)),
 * bf16 activations.  Same arithmetic as three dcpt_conv_ln_fwd_bf16 / dcpt_conv_ln_bwd_bf16 calls (forward: bit-identical), fewer passes:
 * a channels-first LayerNorm (:17-44) runs in the epilogue of the GEMM that produces its input wherever a row fits one column tile (<= 128
 * channels, or 256 on the 256-row kernel), and in backward the two inner LayerNorms ride in the epilogues of the data-gradient GEMMs above
 * them, so the gradients of the two inner activations are never written.  group[0..2] = conv1, conv2, conv3:
 *   w [Cout][Cin][k][k] fp32 and/or its cached operand images (wpacked, dcpt_conv_wpack_bf16_bytes; NULL, 0: packed in the call);
 *   lnw / lnb [Cout] fp32 (lnb of conv1 / conv2 is read by backward too: the inner ReLU masks are recomputed from z);  z (conv output), y (group output; y of group 2 = the block's output) [B][H][W][Cout] bf16 and mu / rstd [B H W]
 *   fp32 are written by forward and read by backward;  dw / dlnw / dlnb: backward outputs (unused in forward).
 * dout, x, dx: [B][H][W][C] bf16.  Workspace: dcpt_bottleneck_bf16_ws_bytes. */
typedef struct {
    const float* w;
    const void* wpacked;
    size_t wpacked_bytes;
    const float* lnw;
    const float* lnb;
    uint16_t* z;
    uint16_t* y;
    float* mu;
    float* rstd;
    float* dw;
    float* dlnw;
    float* dlnb;
} dcpt_bneck_group_t;
size_t dcpt_bottleneck_bf16_ws_bytes(int B, int H, int W, int C, int backward);
int dcpt_bottleneck_fwd_bf16(const uint16_t* x, const dcpt_bneck_group_t* group, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                             dcpt_stream_t stream);
int dcpt_bottleneck_bwd_bf16(const uint16_t* dout, const uint16_t* x, const dcpt_bneck_group_t* group, uint16_t* dx, void* ws, size_t ws_bytes,
                             int B, int H, int W, int C, dcpt_stream_t stream);

/* ABI 15: launch trace for tests.  dcpt_trace_enable(1) clears and starts it: from then on every dispatch decision of the library counts the
 * kernel family it launched under a fixed name ("head.conv3x3+ln_fwd_epilogue", "nt_bf16.256", ...); dcpt_trace_read writes "name count\n"
 * lines into buf (NUL-terminated, truncated to cap) and returns the bytes the whole text needs.  Off (the default) it costs one load per launch.
 * A parity test uses it to assert WHICH kernel produced the result it compared (tests/kernel_trace.py).
 * The fp32 GEMMs name the tile of every launch: "nt_f32.128x64" / "nt_f32.128x96" / "nt_f32.128x128" (BM x BN of launch_gemm_nt),
 * "tn_f32.64x64" / ".128x64" / ".64x128" / ".128x128" / ".128x96" / ".96x128" (the N x K output tile of launch_gemm_tn), and
 * "nt_f32.x3" / "tn_f32.x3" where the opt-in bf16x3 mode takes the launch instead.
 * The fp32 depthwise launches of the Restormer / PromptIR halves name their form: MDTA "dw.reg_plain_fwd_f32" (register kernel, always),
 * backward "dw.ring_plain_bwd_f32" (row ring, 3C % 8 == 0) or "dw.reg_bwd_f32" (register kernel, otherwise); GDFN "dw.ring_gelu_fwd_f32" /
 * "dw.ring_gelu_bwd_f32", and "dw.reg_gelu_fwd_f32" / "dw.reg_gelu_bwd_a_f32" (+ "dw.reg_bwd_f32") for the register forms behind them,
 * which no legal fp32 shape reaches (tests/test_gpu_restormer_halves.py).  Their bf16 twins: "rst_bf16.dw_sq_fwd", "rst_bf16.dw_plain_bwd",
 * "dw.ring_gelu_fwd_bf16", "dw.ring_bwd_gelu_bf16". */
int dcpt_trace_enable(int on);
size_t dcpt_trace_read(char* buf, size_t cap);

/* TLSC variant (nafnet_arch.py:277-288 `NAFNet`, arch_util.py:313-455): inference-only forward where SCA's global
 * mean is a k1 x k2 local box mean (replicate-padded), i.e. a per-pixel attention map.  Callers use the plain
 * dcpt_nafblock_fwd when the window covers the whole map (arch_util.py:352-353). */
size_t dcpt_nafblock_local_ws_bytes(int B, int H, int W, int C, int k1, int k2);
int dcpt_nafblock_local_fwd(const dcpt_nafblock_params* p, const float* inp, float* out, void* ws, size_t ws_bytes, int B, int H,
                            int W, int C, int k1, int k2, dcpt_stream_t stream);

/* The TLSC block in bf16 storage (still ABI 15: purely additive).  Same network semantics as dcpt_nafblock_local_fwd (nafnet_arch.py:277-288
 * `NAFNet`, arch_util.py:313-455; the local mean itself arch_util.py:378-396) on bf16 activations with fp32 parameters: LayerNorm1 -> conv1 and
 * the depthwise + SimpleGate forward as dcpt_nafblock_fwd_bf16 runs them at that width and pixel count, the k1 x k2 box mean of t2 (fp32
 * window sums, one rounding to bf16 after the divide), t2s = bf16((Wsca mean + bsca) * t2) as ONE bf16 GEMM whose epilogue multiplies
 * (one rounding), conv3 with bias / beta / residual, and the second half exactly as the global forward chooses it.  Inference only: nothing
 * is kept.  k1 / k2 are clamped to H / W (arch_util.py:381); callers use the plain dcpt_nafblock_fwd_bf16 when the window covers the
 * whole map (arch_util.py:352-353).  C % 8 == 0, C <= 1024.  `packed`: the block's dcpt_nafblock_wpack_bf16 buffer, or NULL -- the call then
 * packs its weights itself; the operand copy of sca_w is made in the call either way (the pack layout is unchanged).  Workspace too small:
 * DCPT_ERR_WS, nothing launched.  No synchronisation. */
size_t dcpt_nafblock_local_fwd_bf16_ws_bytes(int B, int H, int W, int C, int k1, int k2);
int dcpt_nafblock_local_fwd_bf16(const dcpt_nafblock_params* p, const void* packed, size_t packed_bytes, const uint16_t* inp, uint16_t* out,
                                 void* ws, size_t ws_bytes, int B, int H, int W, int C, int k1, int k2, dcpt_stream_t stream);
/* The box mean of that block on its own (arch_util.py:378-396): out[b][h][w][c] = mean of the k1 x k2 window of `in` (bf16 NHWC) whose
 * top-left corner is (clamp(h - (k1-1)/2, 0, H-k1), clamp(w - (k2-1)/2, 0, W-k2)) -- the (H-k1+1) x (W-k2+1) valid means replicate-padded
 * back to H x W with the smaller pad on the left / top.  k1 / k2 are clamped to H / W.  ws: dcpt_box_mean_bf16_ws_bytes (fp32 row sums). */
size_t dcpt_box_mean_bf16_ws_bytes(int B, int H, int W, int C, int k1, int k2);
int dcpt_box_mean_bf16(const uint16_t* in, uint16_t* out, void* ws, size_t ws_bytes, int B, int H, int W, int C, int k1, int k2,
                       dcpt_stream_t stream);

/* ---- network-edge 3x3 convs ------------------------------------------------------------------
 * intro: nafnet_arch.py:202-210,252  x NCHW [B][Cin][H][W] -> y NHWC [B][H][W][Cout]
 * ending: nafnet_arch.py:211-219,271-272  x NHWC -> y NCHW [B][Cout][H][W] (+ res NCHW, may be NULL) */
int dcpt_conv3x3_in_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin,
                        int Cout, dcpt_stream_t stream);
size_t dcpt_conv3x3_in_bwd_ws_bytes(int B, int H, int W, int Cin, int Cout);
/* dx (NCHW) may be NULL when the image does not need a gradient */
int dcpt_conv3x3_in_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, void* ws,
                        size_t ws_bytes, int B, int H, int W, int Cin, int Cout, dcpt_stream_t stream);
int dcpt_conv3x3_out_fwd(const float* x, const float* w, const float* bias, const float* res, float* y, int B, int H,
                         int W, int Cin, int Cout, dcpt_stream_t stream);
size_t dcpt_conv3x3_out_bwd_ws_bytes(int B, int H, int W, int Cin, int Cout);
int dcpt_conv3x3_out_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, void* ws,
                         size_t ws_bytes, int B, int H, int W, int Cin, int Cout, dcpt_stream_t stream);

/* ---- down: Conv2d(C, 2C, 2, 2) (nafnet_arch.py:230) ------------------------------------------
 * x [B][H][W][C] -> y [B][H/2][W/2][2C];  w [2C][C][2][2] */
size_t dcpt_down2x2_ws_bytes(int B, int H, int W, int C, int backward);
int dcpt_down2x2_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B,
                     int H, int W, int C, dcpt_stream_t stream);
/* dx = dx_add + the data gradient (dx_add NHWC [B][H][W][C] or NULL).  An encoder group's output feeds the down layer AND the skip
 * connection (nafnet_arch.py:255-258, :264-265): the skip's gradient (= the up layer's dy) is summed in the scatter epilogue of the down
 * layer's data-gradient GEMM instead of by a pass of autograd's own over the feature map. */
int dcpt_down2x2_bwd(const float* dy, const float* x, const float* w, const float* dx_add, float* dx, float* dw, float* dbias, void* ws,
                     size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream);

/* ---- up: Conv2d(C, 2C, 1, bias=False) + PixelShuffle(2) + skip add (nafnet_arch.py:238-242,264-265)
 * x [B][H][W][C], skip/y [B][2H][2W][C/2];  w [2C][C][1][1].  The skip gradient equals dy. */
size_t dcpt_up_ps_ws_bytes(int B, int H, int W, int C, int backward);
int dcpt_up_ps_fwd(const float* x, const float* w, const float* skip, float* y, void* ws, size_t ws_bytes, int B, int H,
                   int W, int C, dcpt_stream_t stream);
int dcpt_up_ps_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, void* ws, size_t ws_bytes,
                   int B, int H, int W, int C, dcpt_stream_t stream);

/* ---- degradation-classifier head (basicsr/archs/degrad_classify_arch.py) -------------------------
 * conv (ksize 1 or dense 3x3 / pad 1, no bias, weight [Cout][Cin][k][k]) -> channels-first LayerNorm (eps 1e-6,
 * :17-44) -> [+ res] -> [ReLU]: the `Conv2d` wrapper :69-103 with norm="LN" and the BottleneckBlock tail :227-243.
 * z = conv output (saved for backward), y = result; x,z,y,res NHWC. */
size_t dcpt_conv_ln_ws_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int backward);
int dcpt_conv_ln_fwd(const float* x, const float* w, const float* lnw, const float* lnb, const float* res, int relu, float* z,
                     float* y, float* mu, float* rstd, void* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout,
                     int ksize, dcpt_stream_t stream);
/* dres (may be NULL) receives the gradient of the residual input; dx may be NULL.  dx = dx_add + conv^T(dz) (dx_add NHWC [B][H][W][Cin] or
 * NULL; may alias dx) -- the shortcut gradient of a BottleneckBlock (:227-243) summed in the data-gradient GEMM's epilogue */
int dcpt_conv_ln_bwd(const float* dy, const float* x, const float* w, const float* lnw, const float* z, const float* y,
                     const float* mu, const float* rstd, const float* dx_add, float* dx, float* dw, float* dlnw, float* dlnb, float* dres,
                     void* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout, int ksize, int relu, dcpt_stream_t stream);
/* downsample layer :596-602: Conv2d(Cin, Cout, 1, bias=False) -> MaxPool2d(2,2) -> ReLU; y [B][H/2][W/2][Cout] */
size_t dcpt_conv1x1_pool_relu_ws_bytes(int B, int H, int W, int Cin, int Cout, int backward);
int dcpt_conv1x1_pool_relu_fwd(const float* x, const float* w, float* z, float* y, void* ws, size_t ws_bytes, int B, int H, int W,
                               int Cin, int Cout, dcpt_stream_t stream);
int dcpt_conv1x1_pool_relu_bwd(const float* dy, const float* x, const float* w, const float* z, float* dx, float* dw, void* ws,
                               size_t ws_bytes, int B, int H, int W, int Cin, int Cout, dcpt_stream_t stream);
/* :632-637: out = prev + softmax(mixing_weights)[idx] * feat  (prev may be NULL); the gradient of prev equals dout */
int dcpt_mix_fwd(const float* prev, const float* feat, const float* mixing_weights, int n, int idx, float* out, int64_t numel,
                 dcpt_stream_t stream);
size_t dcpt_mix_bwd_ws_bytes(int64_t numel);
int dcpt_mix_bwd(const float* dout, const float* feat, const float* mixing_weights, int n, int idx, float* dfeat, float* dmix,
                 void* ws, size_t ws_bytes, int64_t numel, dcpt_stream_t stream);
/* downsample=True (:622-637, the SwinIR head; additive, ABI unchanged): stage i mixes the nearest down-sampling of a full-resolution
 * map by s = 2**i, F.interpolate(feature, scale_factor=1/s) of :636, which reads source pixel (h*s, w*s).
 *   out[B][H/s][W/s][C] = prev + softmax(mixing_weights)[idx] * feat[b][h*s][w*s][:]          (prev may be NULL)
 * feat is an NHWC map [B][H][W][C] addressed as feat + b*sb + y*sh + x*sw (element strides of batch, row and pixel; channels are
 * contiguous), so a batch slice of a larger map or an already strided view is read in place; out, prev, dout and dfeat_c are dense.
 * C % 4 == 0, s a power of two that divides H and W, strides multiples of 4, 16-byte aligned pointers.  With s == 1 and dense strides
 * the results equal dcpt_mix_fwd / dcpt_mix_bwd bit for bit.  The backward writes the COMPACT gradient dfeat_c[B][H/s][W/s][C] =
 * softmax[idx] * dout and dmix (per-block partials in a fixed order + one finishing block: no atomics, repeatable bit for bit);
 * workspace dcpt_mix_stride_bwd_ws_bytes(B * (H/s) * (W/s) * C).  The gradient of prev equals dout. */
int dcpt_mix_stride_fwd(const float* prev, const float* feat, const float* mixing_weights, int n, int idx, float* out, int B, int H, int W,
                        int C, int s, int64_t sb, int64_t sh, int64_t sw, dcpt_stream_t stream);
size_t dcpt_mix_stride_bwd_ws_bytes(int64_t numel_coarse);
int dcpt_mix_stride_bwd(const float* dout, const float* feat, const float* mixing_weights, int n, int idx, float* dfeat_c, float* dmix,
                        void* ws, size_t ws_bytes, int B, int H, int W, int C, int s, int64_t sb, int64_t sh, int64_t sw,
                        dcpt_stream_t stream);
/* the backward of that down-sampling (:636) merged into the gradient of the map's other use (the encoder going on after the hook,
 * ...pretrain_model.py:88-91,154-163): g[b][h*s][w*s][:] += dfeat_c[b - lo][h][w][:] for samples lo <= b < hi of the dense NHWC
 * gradient g[B][H][W][C], in place.  dcpt_grid_scatter writes the same into a fresh map in one pass: out[B][H][W][C] = dfeat_c on
 * the grid positions of samples lo..hi-1, zero everywhere else. */
int dcpt_grid_add(float* g, const float* dfeat_c, int B, int lo, int hi, int H, int W, int C, int s, dcpt_stream_t stream);
int dcpt_grid_scatter(const float* dfeat_c, float* out, int B, int lo, int hi, int H, int W, int C, int s, dcpt_stream_t stream);
/* :639-640: mean over the P pixels of each image, then Linear(C, NC).  x [B][P][C] */
size_t dcpt_meanpool_fc_ws_bytes(int B, int P, int C);
int dcpt_meanpool_fc_fwd(const float* x, const float* fw, const float* fb, float* pooled, float* logits, void* ws, size_t ws_bytes,
                         int B, int P, int C, int NC, dcpt_stream_t stream);
int dcpt_meanpool_fc_bwd(const float* dlogits, const float* pooled, const float* fw, float* dx, float* dfw, float* dfb, void* ws,
                         size_t ws_bytes, int B, int P, int C, int NC, dcpt_stream_t stream);
/* ABI 11: the same four with the feature maps (prev / feat / out, dout / dfeat; x, dx) in bf16 storage -- the all-bf16 head
 * (degrad_classify_arch.py:632-640 with act_dtype "bf16") mixes and pools without cast passes.  Arithmetic and reductions are fp32, one
 * rounding on store: the results equal the fp32 entry points' behind casts, bit for bit.  Workspaces as above. */
int dcpt_mix_fwd_bf16(const uint16_t* prev, const uint16_t* feat, const float* mixing_weights, int n, int idx, uint16_t* out, int64_t numel,
                      dcpt_stream_t stream);
int dcpt_mix_bwd_bf16(const uint16_t* dout, const uint16_t* feat, const float* mixing_weights, int n, int idx, uint16_t* dfeat, float* dmix,
                      void* ws, size_t ws_bytes, int64_t numel, dcpt_stream_t stream);
int dcpt_meanpool_fc_fwd_bf16(const uint16_t* x, const float* fw, const float* fb, float* pooled, float* logits, void* ws, size_t ws_bytes,
                              int B, int P, int C, int NC, dcpt_stream_t stream);
int dcpt_meanpool_fc_bwd_bf16(const float* dlogits, const float* pooled, const float* fw, uint16_t* dx, float* dfw, float* dfb, void* ws,
                              size_t ws_bytes, int B, int P, int C, int NC, dcpt_stream_t stream);
/* PromptIR_DC.conv_embed (:491-494, Conv2d(3, dim, 7, 2, 3) + bias -> LayerNorm): the strided conv over the NCHW image is
 * unfolded into patch rows A[(b,oy,ox)][Kp], column k = (c*ksize + ky)*ksize + kx (the weight's own order), column
 * Cin*ksize*ksize = 1 (the bias column), the rest 0 up to Kp (a multiple of 4); the product + LayerNorm then run through
 * dcpt_conv_ln_* as a 1x1 conv over the patch rows.  dcpt_patch_fold is the gradient of the image (gather, fixed order). */
int dcpt_patch_unfold(const float* x, float* A, int B, int Cin, int H, int W, int ksize, int stride, int pad, int Kp,
                      dcpt_stream_t stream);
int dcpt_patch_fold(const float* dA, float* dx, int B, int Cin, int H, int W, int ksize, int stride, int pad, int Kp,
                    dcpt_stream_t stream);

/* plain conv (ksize 1 or dense 3x3 / pad 1, no bias), NHWC -> NHWC: Restormer Downsample/Upsample convs
 * (restormer_arch.py:179-185,194-200) and reduce_chan_level{2,3} (:300-302,:315-317) */
size_t dcpt_conv_ws_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int backward);
int dcpt_conv_fwd(const float* x, const float* w, float* y, void* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout,
                  int ksize, dcpt_stream_t stream);
int dcpt_conv_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, void* ws, size_t ws_bytes, int B, int H,
                  int W, int Cin, int Cout, int ksize, dcpt_stream_t stream);

/* ---- Restormer blocks (basicsr/archs/restormer_arch.py) -------------------------------------------------
 * MDTA half of a TransformerBlock (:148-159 with Attention :103-145):  y = x + project_out(attn(LN(x))).
 * flags: DCPT_LN_BIASFREE = BiasFree_LayerNorm (:26-40, norm_b ignored), else WithBias_LayerNorm (:43-59); 0 / 1 are the
 * Restormer settings of this repo's reference (LayerNorm eps 1e-6, ReLU attention :134-136).  DCPT_LN_EPS_1E5 and
 * DCPT_ATTN_SOFTMAX select the PromptIR variants of the same blocks (basicsr/archs/promptir_arch.py:39-40,57-59: eps 1e-5;
 * :136: softmax over the last dimension).  heads: C % heads == 0 and (C / heads) % 4 == 0 (<= 256 for softmax).
 * F.normalize over the pixels (eps 1e-12). */
#define DCPT_LN_BIASFREE 1
#define DCPT_LN_EPS_1E5 2
#define DCPT_ATTN_SOFTMAX 4
typedef struct {
    const float* norm_w; const float* norm_b;   /* [C] */
    const float* qkv_w;                         /* [3C][C][1][1] */
    const float* dw_w;                          /* [3C][1][3][3] */
    const float* proj_w;                        /* [C][C][1][1] */
    const float* temperature;                   /* [heads][1][1] */
} dcpt_mdta_params;
typedef struct {
    float* norm_w; float* norm_b; float* qkv_w; float* dw_w; float* proj_w; float* temperature;
} dcpt_mdta_params_grads;
typedef struct {   /* saved for backward; M = B*H*W, ch = C/heads */
    float* mu; float* rstd;       /* [M] */
    float* qkv1;                  /* [M][3C] conv1x1(LN(x)) */
    float* qkv;                   /* [M][3C] after the depthwise 3x3 */
    float* nrm;                   /* [B][2C] L2 norms of q and k over the pixels */
    float* ghat; float* attn; float* attnT;   /* [B][heads][ch][ch] */
    float* out_att;               /* [M][C] attn @ v */
    float* xn;                    /* [M][C] LN(x): plain operand of the qkv conv in forward and weight gradient */
    /* LEAN MODE: qkv1, out_att and xn may be NULL (pass the same NULLs to forward and backward): the forward pass then keeps
     * them in the workspace only and the backward pass recomputes them (one LayerNorm pass, the qkv GEMM, the attn @ v GEMM)
     * -- 5 of the 9 [M][C] units this half keeps, for ~8 % more flops. */
} dcpt_mdta_saved;
size_t dcpt_mdta_ws_bytes(int B, int H, int W, int C, int heads, int backward);
int dcpt_mdta_fwd(const dcpt_mdta_params* p, const float* x, float* y, const dcpt_mdta_saved* saved, void* ws, size_t ws_bytes,
                  int B, int H, int W, int C, int heads, int flags, dcpt_stream_t stream);
int dcpt_mdta_bwd(const dcpt_mdta_params* p, const dcpt_mdta_params_grads* g, const float* x, const dcpt_mdta_saved* saved,
                  const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int heads, int flags,
                  dcpt_stream_t stream);
/* GDFN half (:75-100):  y = x + project_out(gelu(x1) * x2), (x1,x2) = dwconv(project_in(LN(x))).chunk(2); the erf GELU of
 * torch.nn.functional.gelu (not the tanh form), evaluated branch-free with |error| <= 5e-7 absolute (Abramowitz-Stegun 7.1.26).
 * hidden = int(C * ffn_expansion_factor) may be any positive integer (padded to a multiple of 4 internally).
 * flags: DCPT_LN_BIASFREE | DCPT_LN_EPS_1E5 as for dcpt_mdta_fwd. */
typedef struct {
    const float* norm_w; const float* norm_b;   /* [C] */
    const float* in_w;                          /* [2*hidden][C][1][1] */
    const float* dw_w;                          /* [2*hidden][1][3][3] */
    const float* out_w;                         /* [C][hidden][1][1] */
} dcpt_gdfn_params;
typedef struct { float* norm_w; float* norm_b; float* in_w; float* dw_w; float* out_w; } dcpt_gdfn_params_grads;
typedef struct {   /* hp = hidden rounded up to a multiple of 4 */
    float* mu; float* rstd;   /* [M] */
    float* u;                 /* [M][2hp] project_in(LN(x)) */
    float* t;                 /* [M][hp]  gelu(x1)*x2 */
    float* xn;                /* [M][C]   LN(x): plain operand of project_in in forward and weight gradient */
    /* LEAN MODE: t and xn may be NULL (in forward AND backward): recomputed in backward from u and x. */
} dcpt_gdfn_saved;
size_t dcpt_gdfn_ws_bytes(int B, int H, int W, int C, int hidden, int backward);
int dcpt_gdfn_fwd(const dcpt_gdfn_params* p, const float* x, float* y, const dcpt_gdfn_saved* saved, void* ws, size_t ws_bytes,
                  int B, int H, int W, int C, int hidden, int flags, dcpt_stream_t stream);
int dcpt_gdfn_bwd(const dcpt_gdfn_params* p, const dcpt_gdfn_params_grads* g, const float* x, const dcpt_gdfn_saved* saved,
                  const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int hidden, int flags,
                  dcpt_stream_t stream);
/* ---- Restormer blocks with bf16 activation storage (restormer_bf16.hip; Restormer / Restormer_origin with act_dtype "bf16") ------
 * The same two halves as dcpt_mdta_* / dcpt_gdfn_* above (reference restormer_arch.py:75-100, :103-145, :148-159), the same parameter
 * structs and flags (DCPT_LN_BIASFREE | DCPT_LN_EPS_1E5 | DCPT_ATTN_SOFTMAX; eps 1e-6, or 1e-5 with the flag); x, y, dy, dx and every
 * [M][.] tensor of the saved structs are bf16 (RNE on store), while mu / rstd, the L2 norms, ghat / attn / attnT, the parameters and
 * all parameter gradients (temperature included) are fp32 and every sum is accumulated in fp32.  No atomics: results are run-to-run
 * bit-identical, and identical across the save modes (the LEAN-mode NULLs of the fp32 structs apply field by field).
 * MDTA: C % heads == 0, ch = C / heads a multiple of 8 and <= 256, C <= 1024 (heads wider than 96 channels run on kernels of their
 *       own, tiled over the head's channels; up to 96 the results are those of ABI 15 as first released).
 * GDFN: C % 8 == 0, C <= 1024; hidden is padded to hp = a multiple of 8 (u [M][2hp], t [M][hp]; pad columns are zero).
 * The *_ws_bytes queries return 0 for a shape the entry points reject; their `backward` argument is 0 / 1 (forward / backward), plus 2
 * when the call will pass every optional saved tensor (MDTA: xn, qkv1, out_att; GDFN: xn, t -- the "full" save mode): the workspace then
 * holds no copies of them. */
typedef struct {   /* field order of dcpt_mdta_saved */
    float* mu; float* rstd;       /* [M] fp32 */
    uint16_t* qkv1;               /* [M][3C] bf16, may be NULL (lean) */
    uint16_t* qkv;                /* [M][3C] bf16 */
    float* nrm;                   /* [B][2C] fp32 */
    float* ghat; float* attn; float* attnT;   /* [B][heads][ch][ch] fp32 */
    uint16_t* out_att;            /* [M][C] bf16, may be NULL */
    uint16_t* xn;                 /* [M][C] bf16, may be NULL */
} dcpt_mdta_saved_bf16;
size_t dcpt_mdta_bf16_ws_bytes(int B, int H, int W, int C, int heads, int backward);
int dcpt_mdta_bf16_fwd(const dcpt_mdta_params* p, const uint16_t* x, uint16_t* y, const dcpt_mdta_saved_bf16* saved, void* ws, size_t ws_bytes,
                       int B, int H, int W, int C, int heads, int flags, dcpt_stream_t stream);
int dcpt_mdta_bf16_bwd(const dcpt_mdta_params* p, const dcpt_mdta_params_grads* g, const uint16_t* x, const dcpt_mdta_saved_bf16* saved,
                       const uint16_t* dy, uint16_t* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int heads, int flags,
                       dcpt_stream_t stream);
typedef struct {   /* field order of dcpt_gdfn_saved; hp = hidden rounded up to a multiple of 8 */
    float* mu; float* rstd;   /* [M] fp32 */
    uint16_t* u;              /* [M][2hp] bf16 */
    uint16_t* t;              /* [M][hp] bf16, may be NULL */
    uint16_t* xn;             /* [M][C] bf16, may be NULL */
} dcpt_gdfn_saved_bf16;
size_t dcpt_gdfn_bf16_ws_bytes(int B, int H, int W, int C, int hidden, int backward);
int dcpt_gdfn_bf16_fwd(const dcpt_gdfn_params* p, const uint16_t* x, uint16_t* y, const dcpt_gdfn_saved_bf16* saved, void* ws, size_t ws_bytes,
                       int B, int H, int W, int C, int hidden, int flags, dcpt_stream_t stream);
int dcpt_gdfn_bf16_bwd(const dcpt_gdfn_params* p, const dcpt_gdfn_params_grads* g, const uint16_t* x, const dcpt_gdfn_saved_bf16* saved,
                       const uint16_t* dy, uint16_t* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int hidden, int flags,
                       dcpt_stream_t stream);
/* the glue between the bf16 blocks (restormer_arch.py:175-202 Down/Upsample, :390-400 skip concat, reduce_chan_level* 1 x 1):
 * dcpt_pixel_(un)shuffle / dcpt_concat_channels / dcpt_split_channels with bf16 elements (concat / split: Ca, Cb % 8 == 0), and the
 * bias-free conv of dcpt_conv_fwd / _bwd (ksize 1 or 3, pad 1) with bf16 x / y / dy / dx, fp32 w / dw (Cin, Cout % 8 == 0, <= 1024). */
int dcpt_pixel_unshuffle_bf16(const uint16_t* x, uint16_t* y, int B, int H, int W, int C, dcpt_stream_t stream);
int dcpt_pixel_shuffle_bf16(const uint16_t* x, uint16_t* y, int B, int H, int W, int C4, dcpt_stream_t stream);
int dcpt_concat_channels_bf16(const uint16_t* a, const uint16_t* b, uint16_t* out, int64_t M, int Ca, int Cb, dcpt_stream_t stream);
int dcpt_split_channels_bf16(const uint16_t* cat, uint16_t* a, uint16_t* b, int64_t M, int Ca, int Cb, dcpt_stream_t stream);
size_t dcpt_conv_bf16_ws_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int backward);
int dcpt_conv_fwd_bf16(const uint16_t* x, const float* w, uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W, int Cin, int Cout,
                       int ksize, dcpt_stream_t stream);
int dcpt_conv_bwd_bf16(const uint16_t* dy, const uint16_t* x, const float* w, uint16_t* dx, float* dw, void* ws, size_t ws_bytes, int B, int H,
                       int W, int Cin, int Cout, int ksize, dcpt_stream_t stream);
/* ---- SwinIR blocks (basicsr/archs/swinir_arch.py; the variant without relative-position bias and without shift mask) -----------
 * Tokens are NHWC rows x [B][H][W][C] (= the reference's (B, L, C) with L = H*W row-major).  LayerNorm eps 1e-5.
 * Attention half (SwinTransformerBlock :319-372 up to the first residual, WindowAttention :142-195):
 *   y = x + proj(WMSA(qkv(LN1(x))))  with windows of window x window tokens on the map rolled by -shift (wrapping, unmasked);
 *   qkv columns (s * heads + h) * head_dim + d (s = q, k, v), softmax(head_dim^-0.5 q k^T) v per (window, head).
 *   Supported: C % 4 == 0, C % heads == 0, head_dim <= 64, window^2 <= 64, H and W multiples of window, 0 <= shift < window.
 * saved may be NULL in forward (nothing kept for backward: inference); backward needs every field. */
typedef struct {
    const float* norm_w; const float* norm_b;   /* [C] */
    const float* qkv_w; const float* qkv_b;     /* [3C][C], [3C] */
    const float* proj_w; const float* proj_b;   /* [C][C], [C] */
} dcpt_swin_attn_params;
typedef struct { float* norm_w; float* norm_b; float* qkv_w; float* qkv_b; float* proj_w; float* proj_b; } dcpt_swin_attn_params_grads;
typedef struct {   /* M = B*H*W */
    float* mu; float* rstd;   /* [M] LayerNorm statistics */
    float* qkv;               /* [M][3C] */
    float* att;               /* [M][C] attention output (proj input) */
    float* lse;               /* [M][heads] per-row log-sum-exp of the scores */
} dcpt_swin_attn_saved;
size_t dcpt_swin_attn_ws_bytes(int B, int H, int W, int C, int heads, int backward);
int dcpt_swin_attn_fwd(const dcpt_swin_attn_params* p, const float* x, float* y, const dcpt_swin_attn_saved* saved, void* ws, size_t ws_bytes,
                       int B, int H, int W, int C, int heads, int window, int shift, dcpt_stream_t stream);
int dcpt_swin_attn_bwd(const dcpt_swin_attn_params* p, const dcpt_swin_attn_params_grads* g, const float* x, const dcpt_swin_attn_saved* saved,
                       const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int heads, int window, int shift,
                       dcpt_stream_t stream);
/* MLP half (:370, Mlp :17-41):  y = x + fc2(gelu(fc1(LN2(x)))), erf GELU; hidden % 4 == 0.  saved may be NULL in forward. */
typedef struct {
    const float* norm_w; const float* norm_b;   /* [C] */
    const float* fc1_w; const float* fc1_b;     /* [hidden][C], [hidden] */
    const float* fc2_w; const float* fc2_b;     /* [C][hidden], [C] */
} dcpt_swin_mlp_params;
typedef struct { float* norm_w; float* norm_b; float* fc1_w; float* fc1_b; float* fc2_w; float* fc2_b; } dcpt_swin_mlp_params_grads;
typedef struct {
    float* mu; float* rstd;   /* [M] */
    float* h;                 /* [M][hidden] fc1 output before the GELU */
} dcpt_swin_mlp_saved;
size_t dcpt_swin_mlp_ws_bytes(int B, int H, int W, int C, int hidden, int backward);
int dcpt_swin_mlp_fwd(const dcpt_swin_mlp_params* p, const float* x, float* y, const dcpt_swin_mlp_saved* saved, void* ws, size_t ws_bytes,
                      int B, int H, int W, int C, int hidden, dcpt_stream_t stream);
int dcpt_swin_mlp_bwd(const dcpt_swin_mlp_params* p, const dcpt_swin_mlp_params_grads* g, const float* x, const dcpt_swin_mlp_saved* saved,
                      const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int hidden, dcpt_stream_t stream);
/* RSTB conv / conv_after_body (:634-640, :1098-1099):  y = res + conv3x3(x) + bias, x / res / y NHWC [B][H][W][C], w [C][C][3][3],
 * zero padding 1.  Backward: dx = conv^T(dy), dw, dbias (the residual's gradient is dy itself). */
size_t dcpt_conv3x3_res_ws_bytes(int B, int H, int W, int C, int backward);
int dcpt_conv3x3_res_fwd(const float* x, const float* w, const float* bias, const float* res, float* y, void* ws, size_t ws_bytes, int B, int H,
                         int W, int C, dcpt_stream_t stream);
int dcpt_conv3x3_res_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, void* ws, size_t ws_bytes, int B,
                         int H, int W, int C, dcpt_stream_t stream);
/* SwinIR's image normalisation (:1064-1065, :1102):  dir 0: y = (x - mean[c]) * r;  dir 1: y = x / r + mean[c].  x, y NCHW
 * [B][C][HW]; mean [C] or NULL (then the same two maps are the backward passes: dy * r and dy / r). */
int dcpt_img_affine(const float* x, const float* mean, float* y, int B, int C, int HW, float r, int dir, dcpt_stream_t stream);
/* ---- RCAN (basicsr/archs/rcan_arch.py) --------------------------------------------------------------------------------------------
 * Feature maps are NHWC [B][H][W][C], C % 4 == 0.  The image normalisation and conv_first / conv_last / the group convs use
 * dcpt_img_affine, dcpt_conv3x3_in_*, dcpt_conv3x3_out_* and dcpt_conv3x3_res_*.
 * RCAB (:32-54, ChannelAttention :9-29):  y = x + res_scale * CA(conv2(relu(conv1(x) + b1)) + b2),
 *   CA(t) = t * sigmoid(W2 relu(W1 mean_hw(t) + b1') + b2') per image and channel; W1 [Cr][C] (the 1x1 conv C -> C/squeeze), W2 [C][Cr],
 *   any Cr >= 1.  saved may be NULL in forward (nothing kept for backward: inference); backward needs every field.  No atomics. */
typedef struct {
    const float* conv1_w; const float* conv1_b;   /* rcab.0: [C][C][3][3], [C] */
    const float* conv2_w; const float* conv2_b;   /* rcab.2: [C][C][3][3], [C] */
    const float* ca1_w; const float* ca1_b;       /* rcab.3.attention.1: [Cr][C] (x 1 x 1), [Cr] */
    const float* ca2_w; const float* ca2_b;       /* rcab.3.attention.3: [C][Cr] (x 1 x 1), [C] */
} dcpt_rcab_params;
typedef struct { float* conv1_w; float* conv1_b; float* conv2_w; float* conv2_b; float* ca1_w; float* ca1_b; float* ca2_w; float* ca2_b; } dcpt_rcab_params_grads;
typedef struct {   /* M = B*H*W */
    float* h;        /* [M][C] relu(conv1(x) + b1) */
    float* t;        /* [M][C] conv2(h) + b2 */
    float* pooled;   /* [B][C] mean_hw(t) */
    float* s;        /* [B][C] channel-attention scale */
} dcpt_rcab_saved;
size_t dcpt_rcab_ws_bytes(int B, int H, int W, int C, int Cr, int backward);   /* 0 for unsupported arguments */
int dcpt_rcab_fwd(const dcpt_rcab_params* p, const float* x, float* y, const dcpt_rcab_saved* saved, void* ws, size_t ws_bytes, int B, int H,
                  int W, int C, int Cr, float res_scale, dcpt_stream_t stream);
int dcpt_rcab_bwd(const dcpt_rcab_params* p, const dcpt_rcab_params_grads* g, const float* x, const dcpt_rcab_saved* saved, const float* dy,
                  float* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C, int Cr, float res_scale, dcpt_stream_t stream);
/* One Upsample stage (arch_util.py Upsample: Conv2d(C, r^2 C, 3, 1, 1) + PixelShuffle(r)), r in {2, 3}:
 *   y = PixelShuffle(r)(conv3x3(x, w) + bias),  x NHWC [B][H][W][C], w [r^2 C][C][3][3], bias [r^2 C], y NHWC [B][rH][rW][C];
 *   y channel c at sub-pixel (i, j) is conv channel c r^2 + i r + j.  Backward: dx, dw, dbias from dy. */
size_t dcpt_conv3x3_ps_ws_bytes(int B, int H, int W, int C, int r, int backward);   /* 0 for unsupported arguments */
int dcpt_conv3x3_ps_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H, int W, int C, int r,
                        dcpt_stream_t stream);
int dcpt_conv3x3_ps_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, void* ws, size_t ws_bytes, int B,
                        int H, int W, int C, int r, dcpt_stream_t stream);
/* ---- RCAN inference on bf16 activation storage (rcan_bf16.hip) ---------------------------------------------------------------------
 * Forward only.  Feature maps are bf16 NHWC [B][H][W][C] (16-byte aligned), C % 8 == 0, C <= 1024; parameters fp32; fp32 accumulation.
 * Every conv takes w [Cout][C][3][3] fp32 and/or its cached operand images (wpacked, dcpt_conv_wpack_bf16_bytes(C, Cout, 3) bytes filled by
 * dcpt_conv_wpack_bf16_multi; NULL, 0: packed in the call -- then w must be given).  Values are rounded to bf16 where they are stored: the
 * weight operand images, h, t, y.  Every *_ws_bytes needs no device and returns 0 for unsupported arguments; arguments are checked before
 * the first launch.  No synchronisation, no global state, no atomics (bit-identical run to run).
 * RCAB (rcan_arch.py:32-54, ChannelAttention :9-29):  y = bf16(x + res_scale * t * s),  h = bf16(relu(conv1(x) + b1)),
 *   t = bf16(conv2(h) + b2),  s = sigmoid(W2 relu(W1 mean_hw(t) + b1') + b2') with the mean taken over the fp32 values of t before their
 *   rounding; pooling, FCs and sigmoid in fp32.  p->conv1_w / conv2_w may be NULL where the packed image is given.  Four launches. */
size_t dcpt_rcab_bf16_ws_bytes(int B, int H, int W, int C, int Cr);
int dcpt_rcab_fwd_bf16(const dcpt_rcab_params* p, const void* wpacked1, size_t wpacked1_bytes, const void* wpacked2, size_t wpacked2_bytes,
                       const uint16_t* x, uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W, int C, int Cr, float res_scale,
                       dcpt_stream_t stream);
/* Group conv / conv_after_body (rcan_arch.py:79-82, :147):  y = bf16(res + conv3x3(x) + bias), one GEMM with the residual in its epilogue. */
size_t dcpt_conv3x3_res_bf16_ws_bytes(int B, int H, int W, int C);
int dcpt_conv3x3_res_fwd_bf16(const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, const float* bias,
                              const uint16_t* res, uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream);
/* One Upsample stage (arch_util.py Upsample), r in {2, 3}:  y = bf16(PixelShuffle(r)(conv3x3(x, w) + bias)), w [r^2 C][C][3][3], bias [r^2 C]
 *   in the conv's own channel order, y [B][rH][rW][C]; one GEMM whose epilogue writes the shuffled image (no intermediate map). */
size_t dcpt_conv3x3_ps_bf16_ws_bytes(int B, int H, int W, int C, int r);
int dcpt_conv3x3_ps_fwd_bf16(const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, const float* bias, uint16_t* y,
                             void* ws, size_t ws_bytes, int B, int H, int W, int C, int r, dcpt_stream_t stream);
/* ---- SwinIR inference on bf16 activation storage (swin_bf16.hip) -------------------------------------------------------------------
 * Forward only, the DCPT variant (no relative-position bias, no shift mask).  PADDED ROWS: token maps are bf16 NHWC rows [M][Cp], M = B*H*W,
 * Cp = C rounded up to a multiple of 8 (184 for 180), Cp <= 256; heads are padded to hdp = head_dim rounded up to a multiple of 8 (32 for
 * 30), hdp <= 64: qkv is [M][3*heads*hdp] with slice (s, h, d) at column (s*heads + h)*hdp + d, the attention output [M][heads*hdp].  Pad
 * columns hold exact zeros everywhere, BY CONSTRUCTION OF THE OPERANDS, which the caller builds once per parameter version: weight operand
 * images (bf16, row-major [N][K]) with zero rows for pad outputs and zero columns for pad inputs, biases and LayerNorm vectors (fp32)
 * zero-padded.  Larger multiples than 8 for Cp / hdp are the caller's choice.  Values are rounded to bf16 where they are stored (operand
 * images, LN output, qkv, P, attention output, proj + residual, fc1 + GELU, fc2 + residual); statistics, scores, softmax and accumulation
 * are fp32.  Every *_ws_bytes needs no device and returns 0 for unsupported arguments; arguments are checked before the first launch.  No
 * synchronisation, no global state, no atomics (bit-identical run to run); a row's result does not depend on the batch around it.
 * LayerNorm on padded rows (nn.LayerNorm, swinir_arch.py:325, :370 norm1 / norm2, PatchEmbed.norm :683-690, SwinIR.norm :964, :1056):
 *   y[m][c] = bf16((x[m][c] - mean_m) * rstd_m * w[c] + b[c]) for c < C, 0 for C <= c < Cp; mean / biased variance in fp32, two-pass, over
 *   the C real channels; w, b [Cp] (only the first C entries are read). */
int dcpt_ln_pad_fwd_bf16(const uint16_t* x, const float* w, const float* b, uint16_t* y, int64_t M, int C, int Cp, float eps,
                         dcpt_stream_t stream);
/* Attention half (SwinTransformerBlock :319-372 up to the first residual, WindowAttention :142-195):
 *   y = bf16(x + proj(WMSA(qkv(LN1(x)))))  in four launches: LayerNorm, qkv GEMM + bias, window kernel, proj GEMM + bias + residual.
 *   Windows of window x window tokens on the map rolled by -shift (wrapping, unmasked) by addressing; per (window, head)
 *   softmax(head_dim^-0.5 q k^T) v on the bf16 matrix pipe, the scale (REAL head_dim = C / heads) applied to the fp32 scores.
 *   Supported: 0 < C <= Cp, Cp % 8 == 0, Cp <= 256, C % heads == 0, C / heads <= hdp <= 64, hdp % 8 == 0, window^2 <= 64, H and W multiples of
 *   window, 0 <= shift < window. */
typedef struct {
    const float* norm_w; const float* norm_b;       /* [Cp] fp32, zero-padded */
    const uint16_t* qkv_w; const float* qkv_b;      /* bf16 [3*heads*hdp][Cp], fp32 [3*heads*hdp]: row (s*heads + h)*hdp + d = reference row s*C + h*hd + d */
    const uint16_t* proj_w; const float* proj_b;    /* bf16 [Cp][heads*hdp] (column h*hdp + d = reference column h*hd + d), fp32 [Cp] */
} dcpt_swin_attn_bf16_params;
size_t dcpt_swin_attn_bf16_ws_bytes(int B, int H, int W, int C, int Cp, int heads, int hdp, int window);
int dcpt_swin_attn_fwd_bf16(const dcpt_swin_attn_bf16_params* p, const uint16_t* x, uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W,
                            int C, int Cp, int heads, int hdp, int window, int shift, dcpt_stream_t stream);
/* MLP half (:370, Mlp :17-41):  y = bf16(x + fc2(gelu(fc1(LN2(x))))), exact erf GELU in the fc1 GEMM's epilogue; three launches.
 *   hidden % 8 == 0 (hidden rows are not padded). */
typedef struct {
    const float* norm_w; const float* norm_b;     /* [Cp] fp32, zero-padded */
    const uint16_t* fc1_w; const float* fc1_b;    /* bf16 [hidden][Cp], fp32 [hidden] */
    const uint16_t* fc2_w; const float* fc2_b;    /* bf16 [Cp][hidden], fp32 [Cp] */
} dcpt_swin_mlp_bf16_params;
size_t dcpt_swin_mlp_bf16_ws_bytes(int B, int H, int W, int C, int Cp, int hidden);
int dcpt_swin_mlp_fwd_bf16(const dcpt_swin_mlp_bf16_params* p, const uint16_t* x, uint16_t* y, void* ws, size_t ws_bytes, int B, int H, int W,
                           int C, int Cp, int hidden, dcpt_stream_t stream);
/* ---- RCAN and SwinIR inference: bf16 maps around an fp32 residual stream (act_dtype "bf16_res32"; rcan_bf16.hip, swin_bf16.hip) ----------
 * The two sections above with ONE map kept in fp32: the residual stream S, the map every residual add reads and writes (RCAN: NHWC
 * [M][C]; SwinIR: padded rows [M][Cp], pad columns exact zeros by construction as above).  Every other map is bf16 as above, and every
 * GEMM / conv operand is bf16: the matrix pipe reads the bf16 image Sb = bf16(S), never S.  S is never rounded: an update whose branch is
 * zero returns S bit for bit.  Restrictions, workspaces (the *_res32_ws_bytes queries answer what the bf16 queries answer), argument
 * checks, determinism and batch consistency as in the two sections above; fp32 rows are 16-byte aligned.
 * RCAN:  conv_first -> S (dcpt_conv3x3_in_fwd), Sb by dcpt_cast_f32_bf16.
 *   RCAB:  h = bf16(relu(conv1(Sb) + b1)),  t = bf16(conv2(h) + b2),  s = the fp32 CA of the fp32 column sums as above;
 *          y = S + res_scale * t * s in fp32,  y_bf16 = bf16(y)  (one pass).  x = S, x_bf16 = Sb; all four maps are required. */
size_t dcpt_rcab_bf16_res32_ws_bytes(int B, int H, int W, int C, int Cr);
int dcpt_rcab_fwd_bf16_res32(const dcpt_rcab_params* p, const void* wpacked1, size_t wpacked1_bytes, const void* wpacked2, size_t wpacked2_bytes,
                             const float* x, const uint16_t* x_bf16, float* y, uint16_t* y_bf16, void* ws, size_t ws_bytes, int B, int H, int W,
                             int C, int Cr, float res_scale, dcpt_stream_t stream);
/* Residual conv (RCAN group conv / conv_after_body, SwinIR RSTB conv / conv_after_body at width Cp):  v = res + conv3x3(x) + bias from the
 *   fp32 accumulator, x bf16 (the stream's image, or a LayerNorm output), res fp32;  y = v (fp32) and / or y_bf16 = bf16(v).  Either output
 *   may be NULL, not both: y only where the next reader is a LayerNorm, both where it is a conv, y_bf16 only where the stream ends
 *   (conv_after_body). */
size_t dcpt_conv3x3_res_bf16_res32_ws_bytes(int B, int H, int W, int C);
int dcpt_conv3x3_res_fwd_bf16_res32(const uint16_t* x, const float* w, const void* wpacked, size_t wpacked_bytes, const float* bias,
                                    const float* res, float* y, uint16_t* y_bf16, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                                    dcpt_stream_t stream);
/* SwinIR:  conv_first -> S at width Cp (dcpt_conv3x3_in_fwd with the zero-padded weight): the fp32 residual of conv_after_body.  With
 *   patch_norm the map that enters the first RSTB is LN(conv_first): a LayerNorm output, i.e. a bf16 storage point as everywhere else, so
 *   the stream through the RSTBs STARTS from that bf16 value (widened exactly by dcpt_cast_bf16_f32) and is never rounded afterwards.
 *   LayerNorm on padded rows with fp32 input: dcpt_ln_pad_fwd_bf16 with x fp32 [M][Cp] -- the same two-pass fp32 statistics over the C real
 *   channels (of the unrounded values), bf16 output, pad outputs 0.  No workspace. */
int dcpt_ln_pad_fwd_bf16_res32(const float* x, const float* w, const float* b, uint16_t* y, int64_t M, int C, int Cp, float eps,
                               dcpt_stream_t stream);
/*   Attention half:  y = x + proj(WMSA(qkv(LN1(x)))) with x, y fp32 [M][Cp]; the four launches of dcpt_swin_attn_fwd_bf16, the proj GEMM
 *   adding the fp32 residual to its fp32 accumulator.  y == x is allowed in both halves (the stream updated in place: the closing GEMM reads
 *   and writes each element of it in one thread, and nothing else reads x after the LayerNorm); a partial overlap is not. */
size_t dcpt_swin_attn_bf16_res32_ws_bytes(int B, int H, int W, int C, int Cp, int heads, int hdp, int window);
int dcpt_swin_attn_fwd_bf16_res32(const dcpt_swin_attn_bf16_params* p, const float* x, float* y, void* ws, size_t ws_bytes, int B, int H, int W,
                                  int C, int Cp, int heads, int hdp, int window, int shift, dcpt_stream_t stream);
/*   MLP half:  y = x + fc2(gelu(fc1(LN2(x)))) with x, y fp32 [M][Cp];  y_bf16 (optional, NULL: not written) = bf16(y), the operand of the RSTB
 *   conv after the last block of an RSTB. */
size_t dcpt_swin_mlp_bf16_res32_ws_bytes(int B, int H, int W, int C, int Cp, int hidden);
int dcpt_swin_mlp_fwd_bf16_res32(const dcpt_swin_mlp_bf16_params* p, const float* x, float* y, uint16_t* y_bf16, void* ws, size_t ws_bytes, int B,
                                 int H, int W, int C, int Cp, int hidden, dcpt_stream_t stream);
/* ---- SwinIR super-resolution tail and the "3conv" residual (basicsr/archs/swinir_arch.py) ---------------------------------------------
 * fp32, NHWC feature maps, implicit-GEMM convs with the LeakyReLU in the GEMM epilogue.  Every *_ws_bytes returns 0 for unsupported
 * arguments.  Backward takes the activation mask from the sign of the saved OUTPUT y (y > 0: 1, else slope; 0 <= slope <= 1).
 * conv_before_upsample (:983-985, :1000-1002; nn.LeakyReLU default slope 0.01) and conv_hr + lrelu (:1100, slope 0.2):
 *   y = lrelu(conv3x3(x, w) + bias, slope),  x [B][H][W][Cin], w [Cout][Cin][3][3], y [B][H][W][Cout], Cin % 4 == Cout % 4 == 0
 *   (slope 1 = the plain biased conv). */
size_t dcpt_conv3x3_act_ws_bytes(int B, int H, int W, int Cin, int Cout, int backward);
int dcpt_conv3x3_act_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H, int W, int Cin,
                         int Cout, float slope, dcpt_stream_t stream);
int dcpt_conv3x3_act_bwd(const float* dy, const float* x, const float* y, const float* w, float* dx, float* dw, float* dbias, void* ws,
                         size_t ws_bytes, int B, int H, int W, int Cin, int Cout, float slope, dcpt_stream_t stream);
/* conv_up1 / conv_up2 of the nearest+conv upsampler (:1085-1099):  y = lrelu(conv3x3(nearest2x(x), w) + bias, slope), x [B][H][W][C],
 * w [C][C][3][3], y [B][2H][2W][C].  The up-sampled map is never written: tap pixel (h', w') of the 2H x 2W grid (zero padding applied
 * there) reads x at (h' >> 1, w' >> 1).  Backward: dgrad on the 2H x 2W grid (workspace) and a 2 x 2 sum. */
size_t dcpt_up2_conv3x3_act_ws_bytes(int B, int H, int W, int C, int backward);
int dcpt_up2_conv3x3_act_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                             float slope, dcpt_stream_t stream);
int dcpt_up2_conv3x3_act_bwd(const float* dy, const float* x, const float* y, const float* w, float* dx, float* dw, float* dbias, void* ws,
                             size_t ws_bytes, int B, int H, int W, int C, float slope, dcpt_stream_t stream);
/* UpsampleOneStep (:771-787):  y = PixelShuffle(r)(conv3x3(x, w) + bias) as the NCHW image [B][Cimg][rH][rW], x [B][H][W][C],
 * w [r^2 Cimg][C][3][3], r in {2, 3, 4}, Cimg <= 4; conv channel c r^2 + i r + j is image channel c at sub-pixel (i, j). */
size_t dcpt_conv3x3_ps_out_ws_bytes(int B, int H, int W, int C, int Cimg, int r, int backward);
int dcpt_conv3x3_ps_out_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                            int Cimg, int r, dcpt_stream_t stream);
int dcpt_conv3x3_ps_out_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, void* ws, size_t ws_bytes,
                            int B, int H, int W, int C, int Cimg, int r, dcpt_stream_t stream);
/* RSTB conv / conv_after_body with resi_connection="3conv" (:608-616, :969-977), Cq = C / 4, C % 16 == 0, both slopes 0.2:
 *   a1 = lrelu(conv3x3(x, w1) + b1) [M][Cq],  a2 = lrelu(a1 W2^T + b2) [M][Cq],  y = res + conv3x3(a2, w3) + b3.
 * Forward writes a1 / a2 for backward (both NULL: keep nothing).  Backward: dx and the six parameter gradients; the residual's
 * gradient is dy itself. */
typedef struct {
    const float* conv1_w; const float* conv1_b;   /* conv.0: [Cq][C][3][3], [Cq] */
    const float* conv2_w; const float* conv2_b;   /* conv.2: [Cq][Cq] (x 1 x 1), [Cq] */
    const float* conv3_w; const float* conv3_b;   /* conv.4: [C][Cq][3][3], [C] */
} dcpt_conv3conv_params;
typedef struct { float* conv1_w; float* conv1_b; float* conv2_w; float* conv2_b; float* conv3_w; float* conv3_b; } dcpt_conv3conv_params_grads;
size_t dcpt_conv3conv_res_ws_bytes(int B, int H, int W, int C, int backward);
int dcpt_conv3conv_res_fwd(const dcpt_conv3conv_params* p, const float* x, const float* res, float* y, float* a1, float* a2, void* ws,
                           size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream);
int dcpt_conv3conv_res_bwd(const dcpt_conv3conv_params* p, const dcpt_conv3conv_params_grads* g, const float* x, const float* a1,
                           const float* a2, const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int H, int W, int C,
                           dcpt_stream_t stream);
/* PromptIR's PromptGenBlock (basicsr/archs/promptir_arch.py:237-262) between its linear layer and its 3x3 conv:
 *   out[b] = bilinear_{(S,S)->(H,W), align_corners=False}( sum_l softmax(logits[b])[l] * param[l] )   as NHWC [B][H][W][D].
 * logits [B][L] (= dcpt_meanpool_fc_fwd of the block input), param [L][D][S][S] (the (1,L,D,S,S) parameter), weights [B][L]
 * receives the softmax (saved for backward).  L <= 8, D % 4 == 0. */
int dcpt_prompt_mix_fwd(const float* logits, const float* param, float* weights, float* out, int B, int L, int D, int S, int H, int W,
                        dcpt_stream_t stream);
size_t dcpt_prompt_mix_bwd_ws_bytes(int B, int D, int S);
int dcpt_prompt_mix_bwd(const float* dout, const float* param, const float* weights, float* dlogits, float* dparam, void* ws,
                        size_t ws_bytes, int B, int L, int D, int S, int H, int W, dcpt_stream_t stream);
/* The same with the NHWC map in bf16 (PromptIR with act_dtype="bf16"): out / dout [B][H][W][D] bf16, D % 8 == 0; logits, weights,
 * param, dlogits, dparam fp32; workspace dcpt_prompt_mix_bwd_ws_bytes. */
int dcpt_prompt_mix_fwd_bf16(const float* logits, const float* param, float* weights, uint16_t* out, int B, int L, int D, int S, int H, int W,
                             dcpt_stream_t stream);
int dcpt_prompt_mix_bwd_bf16(const uint16_t* dout, const float* param, const float* weights, float* dlogits, float* dparam, void* ws,
                             size_t ws_bytes, int B, int L, int D, int S, int H, int W, dcpt_stream_t stream);
/* NHWC PixelUnshuffle(2): x [B][H][W][C] -> y [B][H/2][W/2][4C];  PixelShuffle(2): x [B][H][W][C4] -> y [B][2H][2W][C4/4] */
int dcpt_pixel_unshuffle(const float* x, float* y, int B, int H, int W, int C, dcpt_stream_t stream);
int dcpt_pixel_shuffle(const float* x, float* y, int B, int H, int W, int C4, dcpt_stream_t stream);
/* channel concat of two NHWC maps ([M][Ca], [M][Cb] -> [M][Ca+Cb]) and its inverse */
int dcpt_concat_channels(const float* a, const float* b, float* out, int64_t M, int Ca, int Cb, dcpt_stream_t stream);
int dcpt_split_channels(const float* cat, float* a, float* b, int64_t M, int Ca, int Cb, dcpt_stream_t stream);

/* ---- fused bias + leaky-ReLU (API parity with basicsr/ops/fused_act/src/fused_bias_act.cpp:14-26,
 * kernel fused_bias_act_kernel.cu:20-50): y = act(x + bias[(i / step_b) % size_b]) * scale, act in
 * {1: linear, 3: leaky relu(alpha)}; grad 0: forward, 1: first derivative w.r.t. x using `ref` sign. */
int dcpt_fused_bias_act(const float* x, const float* bias, const float* ref, float* y, int64_t n, int size_b,
                        int64_t step_b, int act, int grad, float alpha, float scale, dcpt_stream_t stream);

/* ---- validation metrics: the sums behind PSNR and SSIM, on the device ----------------------------------
 * replaces the host arithmetic of basicsr/metrics/psnr_ssim.py:11-75 (calculate_psnr), :113-183 (calculate_ssim) and :483-512 (_ssim)
 * for a batch of image pairs that is already on the device.  img, img2: dense NCHW fp32 [B][C][H][W] with values in [0, 1], C in {1, 3}.
 * Per element, as the reference does it: rintf(x * 255) in fp32 (round half to even; skipped with DCPT_METRIC_RANGE1), crop_border
 * pixels dropped on every side by addressing, with DCPT_METRIC_Y and C == 3 the BT.601 luma ((24.966 b + 128.553 g + 65.481 r + 16) / 255
 * in fp64 on value / image_range, rounded to fp32, times image_range) as ONE channel; then
 *   sse_out[B]      the sum of squared differences of image b over its channels: int64 (exact) on the quantised RGB / gray path, i.e.
 *                   image_range 255 without luma; fp64 on the luma and DCPT_METRIC_RANGE1 paths;
 *   ssim_out[B][C'] fp64, the sum of the SSIM map (11-tap Gaussian, sigma 1.5, "valid" window, C1 = (0.01 L)^2, C2 = (0.03 L)^2, all in
 *                   fp64) over its (H' - 10) x (W' - 10) positions, H' = H - 2 crop_border; C' = 1 for luma, C otherwise.  Written only
 *                   with DCPT_METRIC_SSIM (may be NULL without it).
 * The host divides by the counts and takes the logarithm.  Two launches on `stream`, no atomics: the same input gives the same bits.
 * Errors (before any launch): null pointers, C not in {1, 3}, unknown flag bits, a cropped size <= 0, a cropped size under 11 with
 * DCPT_METRIC_SSIM, workspace too small.  dcpt_imgmetric_ws_bytes needs no device and returns 0 for arguments dcpt_imgmetric refuses. */
#define DCPT_METRIC_Y 1       /* test_y_channel */
#define DCPT_METRIC_SSIM 2    /* also the SSIM sums */
#define DCPT_METRIC_RANGE1 4  /* image_range = 1 (no quantisation); without it image_range = 255 */
size_t dcpt_imgmetric_ws_bytes(int B, int C, int H, int W, int crop_border, int flags);
int dcpt_imgmetric(const float* img, const float* img2, void* sse_out, double* ssim_out, void* ws, size_t ws_bytes, int B, int C, int H, int W,
                   int crop_border, int flags, dcpt_stream_t stream);

/* ---- validation metrics: MS-SSIM, MATLAB SSIM and the NRMSE range, on the device -------------------------
 * img, img2, crop_border, the front end and the flags DCPT_METRIC_Y / DCPT_METRIC_RANGE1 as for dcpt_imgmetric (DCPT_METRIC_SSIM is not
 * taken); C' = 1 for luma, C otherwise; H' = H - 2 crop_border.  All window arithmetic is fp64, every product and sum rounds on its own.
 *   dcpt_msssim       replaces basicsr/metrics/psnr_ssim.py:334-432 (calculate_msssim) with its _ssim (:483-512) and its cv2.filter2D box
 *                     blurs (:410-423).  out[B][levels][2] = for evaluation k the sums of the SSIM map and of the CS map
 *                     (2 s12 + C2) / (s1 + s2 + C2) over the (H' - 10) x (W' - 10) "valid" positions of channel k mod C' of both images after
 *                     k passes of out[y][x] = 0.25 ((a[y][x] + a[y][x+1]) + (a[y+1][x] + a[y+1][x+1])), an index past the last row / column
 *                     reading the last one (the reference does not decimate, and blurs inside its channel loop).  The host divides by the
 *                     count and forms prod(cs_k ^ w_k) ssim_{L-1} ^ w_{L-1}.  One launch over (tile, image, level) + one reduce.
 *   dcpt_ssim_matlab  replaces :201-330 (SSIM_MATLAB_Pytorch, calculate_ssim_matlab): out[B][C'] = the sum over all H' x W' pixels of
 *                     ((2 mu12 + C1) (2 s12 + C2)) / ((mu1^2 + mu2^2 + C1) (s1 + s2 + C2)), the 11 x 11 window under replicate padding of
 *                     5; any H', W' >= 1.  fp64 where the reference's Conv2d is fp32.  The host divides by H' W' and doubles the last channel.
 *   dcpt_imgrange     replaces img.max() - img.min() of :563-612 (calculate_nrmse): out[B][2] = the minimum and the maximum of image b's
 *                     scored values (exact fp32 numbers, stored as fp64); the squared error comes from dcpt_imgmetric.
 * Two launches each on `stream`, no atomics: the same input gives the same bits.  Errors (before any launch): null pointers, C not in
 * {1, 3}, crop_border < 0, unknown flag bits, a cropped size <= 0, for dcpt_msssim a cropped size under 11 x 11 or levels outside 1 .. 8,
 * B * C (* levels) above 65535, workspace too small.  The *_ws_bytes need no device and return 0 for arguments the entry point refuses. */
size_t dcpt_msssim_ws_bytes(int B, int C, int H, int W, int crop_border, int flags, int levels);
int dcpt_msssim(const float* img, const float* img2, double* out, void* ws, size_t ws_bytes, int B, int C, int H, int W, int crop_border,
                int flags, int levels, dcpt_stream_t stream);
size_t dcpt_ssim_matlab_ws_bytes(int B, int C, int H, int W, int crop_border, int flags);
int dcpt_ssim_matlab(const float* img, const float* img2, double* out, void* ws, size_t ws_bytes, int B, int C, int H, int W, int crop_border,
                     int flags, dcpt_stream_t stream);
size_t dcpt_imgrange_ws_bytes(int B, int C, int H, int W, int crop_border, int flags);
int dcpt_imgrange(const float* img, double* out, void* ws, size_t ws_bytes, int B, int C, int H, int W, int crop_border, int flags,
                  dcpt_stream_t stream);

/* ---- SSIM as a training loss: per-image SSIM sums and their gradient, on the device ------------------------
 * replaces the fp64 arithmetic of basicsr/metrics/psnr_ssim.py:436-480 (calculate_ssim_pt) and :515-559 (_ssim_pth: five grouped 11 x 11
 * fp64 F.conv2d passes, and their transposes under autograd) as the losses of basicsr/losses/basic_loss.py:152-232 (SSIMLoss, SSIMMSELoss)
 * call it.  pred, target: dense NCHW fp32 [B][C][H][W], C in {1, 3}.  crop_border pixels are dropped on every side by addressing; with
 * DCPT_METRIC_Y and C == 3 both images become ONE luma channel, Y = (((r 65.481f + g 128.553f) + b 24.966f) + 16.0f) / 255.0f with every
 * product, sum and the division rounded to fp32 in this order (basicsr/utils/color_util.py:222-254 rgb2ycbcr_pt(y_only=True), an fp32
 * matmul there); the values are widened to fp64 and everything after that is fp64: 11-tap Gaussian (sigma 1.5), "valid" window,
 * C1 = (0.01 image_range)^2, C2 = (0.03 image_range)^2.  C' = 1 for luma, C otherwise; the map has (H' - 10) x (W' - 10) positions,
 * H' = H - 2 crop_border.
 *   dcpt_ssim_loss_fwd   ssim_sum[B][C'] = the sum of the SSIM map of (image, channel); the caller divides by the count (the reference's
 *                        ssim_map.mean([1, 2, 3])).  Two launches.
 *   dcpt_ssim_loss_bwd   dpred[B][C][H][W] = the gradient of sum_{b,c'} gscale[b][c'] * ssim_sum[b][c'] with respect to pred, rounded once
 *                        to fp32; gscale is a DEVICE array, nothing is read back.  Every element is written: pixels inside the crop border
 *                        get exactly 0; with luma the three channels get dY * (65.481f, 128.553f, 24.966f) / 255, formed in fp64.  Two
 *                        launches per chunk of whole images: the workspace holds three fp64 planes per map (24 bytes per position) for at
 *                        most max(one image, 64 MiB) at a time.  target gets no gradient.
 * No atomics: the same input gives the same bits.  Errors (before any launch): null pointers, C not in {1, 3}, a flag other than
 * DCPT_METRIC_Y, image_range <= 0, a cropped size under 11 x 11, B * C above 65535, workspace too small.  dcpt_ssim_loss_ws_bytes needs no
 * device and returns 0 for arguments the entry points refuse. */
size_t dcpt_ssim_loss_ws_bytes(int B, int C, int H, int W, int crop_border, int flags, int backward);
int dcpt_ssim_loss_fwd(const float* pred, const float* target, double* ssim_sum, void* ws, size_t ws_bytes, int B, int C, int H, int W,
                       int crop_border, int flags, double image_range, dcpt_stream_t stream);
int dcpt_ssim_loss_bwd(const float* pred, const float* target, const double* gscale, float* dpred, void* ws, size_t ws_bytes, int B, int C,
                       int H, int W, int crop_border, int flags, double image_range, dcpt_stream_t stream);

/* ---- LDL artifact weights: the refined artifact map and its gradient, on the device ----------------------
 * replaces basicsr/losses/loss_util.py:100-130 (get_local_weights: F.pad(reflect), unfold(7).unfold(7), torch.std, the standardisation and
 * the tanh) and :133-165 (get_refined_artifact_map) on the one path basicsr/models/sr_model.py:145-153 reaches -- std=True, ksize 7, no
 * img_ema -- together with what autograd does to those lines.  gt, out: dense NCHW fp32 [B][C][H][W], N = B C H W.  The window is 7 x 7
 * and nothing else.
 *     r = |gt - out|;  u = unbiased std of r over the 7 x 7 window around each pixel, r reflect-padded by 3;
 *     m = mean(u), s = unbiased std(u) over all N elements;  w = (tanh((u - m) / s) + 1) / 2
 * All of it in fp64; the one departure from the reference: r is |double(gt) - double(out)|, the exact difference, where the reference
 * rounds the difference to fp32 first.
 *   dcpt_ldl_weight_fwd   w[B][C][H][W] fp32, rounded once.  Five launches.  It leaves m, s and the fp64 planes u and mu (the window mean)
 *                         in ws.  out == gt everywhere gives s = 0 and w = NaN everywhere, as the reference's expression does.
 *   dcpt_ldl_weight_bwd   dout[B][C][H][W] fp32 = the gradient with respect to out of sum(gw * w), gw [B][C][H][W] fp32 on the device,
 *                         rounded once.  Four launches.  It READS what the forward left: ws must be the buffer dcpt_ldl_weight_fwd wrote
 *                         for the same gt and out, untouched since, and at least dcpt_ldl_weight_ws_bytes(.., backward = 1) bytes (the
 *                         forward's layout is a prefix of the backward's).  The state is this argument; the library keeps none.  gt gets
 *                         no gradient.
 * m, s and the two global sums of the backward stay in ws: nothing is read back, no call synchronises.  No atomics, every sum in a fixed
 * order: the same input gives the same bits.  Errors (before any launch): null pointers, B C H W < 2, H < 4 or W < 4 (reflect padding by
 * 3), B * C above 65535, a plane above 2^30 pixels, workspace too small (return code 2).  dcpt_ldl_weight_ws_bytes needs no device and
 * returns 0 for a shape the entry points refuse. */
size_t dcpt_ldl_weight_ws_bytes(int B, int C, int H, int W, int backward);
int dcpt_ldl_weight_fwd(const float* gt, const float* out, float* w, void* ws, size_t ws_bytes, int B, int C, int H, int W,
                        dcpt_stream_t stream);
int dcpt_ldl_weight_bwd(const float* gt, const float* out, const float* gw, float* dout, void* ws, size_t ws_bytes, int B, int C, int H,
                        int W, dcpt_stream_t stream);

/* ---- DiffJPEG: the JPEG round trip of a batch, on the device -------------------------------------------
 * replaces basicsr/utils/diffjpeg.py:494-523 (DiffJPEG.forward) with everything it calls: the zero padding to a multiple of 16 (:509-515),
 * x * 255 and RGB -> YCbCr (:59-85, :256), the 2 x 2 chroma mean (:88-119), block splitting and the 8 x 8 DCT of v - 128 with the
 * alpha / 4 scale (:122-171), the division by table * factor with the transposed luma table and the chroma table (:15-34, :174-231),
 * factor = quality_to_factor(quality[b]) per image (:42-55, evaluated in the kernel: 50 / q below 50, 2 - q / 50 from 50 on), the rounding
 * (torch.round, or with DCPT_JPEG_DIFF_ROUND diff_round, :37-39: round(t) + (t - round(t))^3), the dequantisation (:273-318), the iDCT
 * + 128 (:321-346), block merging, the 2 x 2 chroma repeat (:349-398), YCbCr -> RGB (:401-423), the clamp to [0, 255] and / 255
 * (:467-470) and the crop (:519); C == 1 uses the plane as all three channels and returns the mean of the three decoded channels
 * (:507-508, :521-522).  With DCPT_JPEG_UINT8_IO the input is first put on the 8-bit grid, rint(x * 255), and the output is
 * rint(clamped) / 255: what basicsr/data/paired_image_dataset.py:539-546 gets from cv2.imencode / imdecode of the rounded image (with
 * C == 1, rint of the mean of the three clamped channels).
 *   x, y      dense NCHW fp32 [B][C][H][W] in [0, 1] -- the layout of lq / gt, not the NHWC of the feature maps; C = 1 or 3
 *   quality   [B] fp32 on the device, one value per image; it is read, never written (the reference overwrites it with the factors)
 * One launch; one read of x and one write of y; the pad is addressed, never stored.  fp64 from the pixel load to the one rounding to
 * fp32 at the store, so the rounding of a coefficient never hinges on an fp32 summation order; the one departure from the reference: its
 * fp32 pipeline can round a coefficient the other way when the exact value lies within about 1e-4 of a tie.  No workspace, no atomics, no
 * host synchronisation, no global state; an image's result does not depend on the batch around it; the same input gives the same bits.
 * Errors (before the launch): null pointers, non-positive sizes, C not 1 or 3, unknown flag bits, B above 65535, a plane above 2^30
 * pixels. */
#define DCPT_JPEG_DIFF_ROUND 1   /* differentiable=True: the cubic rounding */
#define DCPT_JPEG_UINT8_IO 2     /* 8-bit input and output grids */
int dcpt_diffjpeg_fwd(const float* x, const float* quality, float* y, int B, int C, int H, int W, int flags, dcpt_stream_t stream);

/* ---- MATLAB-bicubic resize and the pixel work of NIQE, on the device ------------------------------------
 * Three entry points in fp64 from the pixel load to the store.  No atomics, every sum in a fixed order (two runs give the same bits), a
 * plane's result does not depend on the planes around it, no host synchronisation, no global state; arguments are checked before the
 * first launch.
 *
 * dcpt_imresize_fwd replaces basicsr/utils/matlab_functions.py:89-186 (imresize) for tables the host built as
 * calculate_weights_indices does (:17-86): the H pass (:148-155), then the W pass (:172-177), the symmetric padded copies (:135-146,
 * :159-170) being addressing only (index -1 -> 0, -2 -> 1, n -> n - 1, ...; an index that would still leave the plane is clamped to it).
 *   x          planes [P][H][W], fp32 or fp64 (DCPT_IMRESIZE_X_F64); plane p starts at x + p * plane_stride elements and its rows are
 *              row_stride elements apart (dense: H * W and W), so a crop is a pointer offset.  With DCPT_IMRESIZE_QUANT8 (fp32 only) a
 *              tap reads rint(255 x) / 255: the 8-bit image / 255.0 of niqe.py:144.
 *   y          dense [P][Ho][Wo], fp32 or fp64 (DCPT_IMRESIZE_Y_F64); the one rounding is at this store
 *   first_h/w  int32 [Ho] / [Wo] on the device: the first tap of an output row / column; may be negative or reach past the end
 *   w_h / w_w  fp64 [Ho][Kh] / [Wo][Kw] on the device: the weights; zero-weight taps are harmless
 *   ws         dcpt_imresize_ws_bytes: the fp64 intermediate [P][Ho][W] (0 for arguments the entry point refuses; needs no device)
 * Errors: null pointers, non-positive sizes, tap counts outside 1..4096, a plane above 2^30 pixels, above 2^36 elements, unknown flags,
 * QUANT8 on an fp64 source, strides under the plane's extent, a workspace that is too small.
 *
 * dcpt_niqe_mscn_fwd replaces niqe.py:121-129 (mu, sigma and the normalised image of one scale) with the crop to whole blocks (:114-117):
 *   scale 1    x fp32 [P][H][W] in [0, 1]; the region starts at (crop_border, crop_border) and is Hc x Wc with
 *              Hc = (H - 2 crop_border) / 96 * 96, Wc likewise; a pixel is rint(255 x), half to even (niqe.py:218)
 *   scale 2    x fp64 [P][H][W], the resize output of niqe.py:144, read as 255 x (:145); H and W multiples of 48, crop_border 0
 *   n          fp64 [P][Hc][Wc]
 * The 7 x 7 window exp(-(i^2 + j^2) / (2 (7/6)^2)), normalised, is computed, the borders replicate the region's edge pixel
 * (mode="nearest"), and the moments are taken around the window's centre pixel p: mu = p + sum w (x - p), var = sum w (x - p)^2 -
 * (mu - p)^2, n = (p - mu) / (sqrt|var| + 1): a constant window gives n = 0 exactly.
 *
 * dcpt_niqe_block_stats_fwd replaces the sums of niqe.py:24-37 (estimate_aggd_param) over the five maps of :56-66 (compute_feature) for
 * every block of :132-139:
 *   n          fp64 [P][H][W], H and W multiples of block (96 at scale 1, 48 at scale 2)
 *   stats      fp64 [P][nblk][5][6], blocks column-major (index idx_w * (H / block) + idx_h); maps: the block, then its product with
 *              np.roll(block, s, axis=(0, 1)) for s = [0, 1], [1, 0], [1, 1], [1, -1], the roll wrapping inside the block; values:
 *              count of x < 0, sum of x^2 over them, count of x > 0, sum of x^2 over them, sum |x| and sum x^2 over all
 * Errors of both: null pointers, bad shape, a scale other than 1 / 2 or a block other than 96 / 48, planes without whole blocks, above
 * 65535 planes, a plane above 2^30 pixels. */
#define DCPT_IMRESIZE_X_F64 1    /* x is fp64 (else fp32) */
#define DCPT_IMRESIZE_Y_F64 2    /* y is fp64 (else fp32) */
#define DCPT_IMRESIZE_QUANT8 4   /* a tap reads rint(255 x) / 255 */
size_t dcpt_imresize_ws_bytes(int P, int H, int W, int Ho, int Wo, int Kh, int Kw);
int dcpt_imresize_fwd(const void* x, void* y, const int* first_h, const double* w_h, const int* first_w, const double* w_w, void* ws,
                      size_t ws_bytes, int P, int H, int W, int Ho, int Wo, int Kh, int Kw, int64_t plane_stride, int64_t row_stride,
                      int flags, dcpt_stream_t stream);
int dcpt_niqe_mscn_fwd(const void* x, double* n, int P, int H, int W, int crop_border, int scale, dcpt_stream_t stream);
int dcpt_niqe_block_stats_fwd(const double* n, double* stats, int P, int H, int W, int block, dcpt_stream_t stream);

/* ---- on-the-fly degradations: demosaic and line-mask inpainting, on the device ---------------------------
 * dcpt_demosaic_fwd replaces basicsr/utils/mosaic_util.py dm_matlab (default) and dm (DCPT_DEMOSAIC_BILINEAR), with the Bayer mosaic of
 * mosaic_CFA_Bayer fused in front of them when C == 3.
 *   x   dense NCHW fp32 [B][C][H][W]: C == 3 an RGB image, of which the kernel reads the CFA sample only -- R at (even row, even column),
 *       B at (odd, odd), G elsewhere (RGGB, masks_CFA_Bayer); C == 1 the CFA plane itself
 *   y   dense NCHW fp32 [B][3][H][W]; a different buffer than x (a pixel reads its neighbours)
 * Default, Malvar-He-Cutler on the CFA plane reflect-padded by 2 (-1 -> 1, -2 -> 2, H -> H - 2, H + 1 -> H - 3).  Taps in units of 1/16:
 *   kgrb    G at an R or B site:  centre 8, the four axis neighbours at distance 1: 4, at distance 2: -2
 *   krbg0   R at (even, odd) and B at (odd, even):  centre 10, left / right 8, two left / right -2, two up / down 1, diagonals -2
 *   krbg0'  (transposed) R at (odd, even) and B at (even, odd)
 *   krbbr   R at a B site and B at an R site:  centre 12, diagonals 4, the axis neighbours at distance 2: -3
 *   the sample the CFA holds passes through
 * DCPT_DEMOSAIC_BILINEAR: 3 x 3 taps on the three sparse colour planes with circular padding, in units of 1/4: R and B
 * (2 - |dy|) (2 - |dx|), G centre 4 and the four axis neighbours 1; a neighbour counts for the colour of the position it wraps to.
 * Without DCPT_DEMOSAIC_UINT8_IO y = sum w x in fp32 on the raw x, no clamp, no rounding (what dm_matlab / dm return; the weights are
 * dyadic, so a Malvar output is a 13-term fp32 sum: within 13 * 2^-24 * 2.5 * max|x|).  With it the arithmetic is integer and exact:
 * v = rint(clamp(x, 0, 1) * 255) with the product in fp32, S = sum tap * v, y = float(rint(clamp(S / 16, 0, 255))) / 255.0f (S / 4 for
 * bilinear), rint half to even: the 8-bit image a camera pipeline would hand on, divided by 255.
 * Odd H and W are supported, an extension: the reference's mosaic_CFA_Bayer refuses them.
 * One launch, no workspace, no atomics, no host synchronisation; the same input gives the same bits.
 * Errors (before the launch): null pointers, x == y, C not 1 or 3, H or W below 3 (the reflection needs 3), B outside 1..65535, a plane
 * above 2^30 pixels, unknown flag bits.
 *
 * dcpt_inpaint_lines_fwd replaces PairedImageInpaintingDataset.inpainting (basicsr/data/paired_image_dataset.py:1009-1029) once the strokes
 * are drawn: the mask of up to 10 thick line segments and np.clip(img +- mask, 0, 1).
 *   x, y    dense NCHW fp32 [B][C][H][W], C = 1 or 3; x == y (in place) is allowed
 *   lines   int32 [B][10][4] on the device: x1, y1, x2, y2 of each stroke (column, row)
 *   meta    int32 [B][3] on the device: n_lines, thick, white
 * A pixel p = (px, py) is masked when it lies within thick / 2 of one of the first n_lines segments, decided in exact 64-bit integers with
 * q = p - P1, d = P2 - P1, a = q . d, L = d . d:  a <= 0: 4 |q|^2 <= thick^2 (also L = 0);  a >= L: 4 |q - d|^2 <= thick^2;  otherwise
 * 4 (q x d)^2 <= thick^2 L.  A masked pixel becomes 1 if white, else 0, in every channel; every other pixel clamp(x, 0, 1).  This is the
 * ideal shape of cv2.polylines with a thickness (a quad plus round caps); the two have not been compared.
 * The entry point cannot see lines and meta without a synchronisation, so the kernel CLAMPS them: n_lines to 0..10, thick to 1..64, an
 * endpoint coordinate to -16384..16384 (which keeps 4 (q x d)^2 inside 64 bits).  Validate them on the host where they are host data.
 * Errors (before the launch): null pointers, non-positive sizes, C not 1 or 3, H or W above 16384, B above 65535. */
#define DCPT_DEMOSAIC_BILINEAR 1   /* dm (bilinear, circular padding) instead of dm_matlab (Malvar, reflect padding) */
#define DCPT_DEMOSAIC_UINT8_IO 2   /* 8-bit input and output grids, integer arithmetic */
int dcpt_demosaic_fwd(const float* x, float* y, int B, int C, int H, int W, int flags, dcpt_stream_t stream);
int dcpt_inpaint_lines_fwd(const float* x, const int* lines, const int* meta, float* y, int B, int C, int H, int W, dcpt_stream_t stream);

/* ---- on-the-fly degradations: Gaussian noise from a counter-based generator, on the device ---------------------
 * dcpt_gauss_noise_fwd replaces the Gaussian family of basicsr/data/degradations.py:530-634 (generate_ / add_ / random_generate_ /
 * random_add_gaussian_noise_pt) and the noise of PairedImageDenoiseDataset (basicsr/data/paired_image_dataset.py:390-402) with one launch
 * for the batch.  The reference draws from torch.randn / np.random.normal, sequential generators that cannot be restated in parallel; the
 * stream here is Philox4x32-10, so results match the reference's in distribution and not in value.
 *   x       dense NCHW fp32 [B][C][H][W]; unused and may be null with DCPT_NOISE_ONLY
 *   sigma   fp32 [B] on the device: the standard deviation of image b on the 0..255 scale
 *   key     int64 [B] on the device: the Philox key of image b (words: its low and its high 32 bits)
 *   gray    int32 [B] on the device or null: non-zero gives image b one noise plane shared by its channels
 *   y       dense NCHW fp32 [B][C][H][W]; y == x (in place) is allowed
 * Generator: Philox4x32-10, multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, counter (q, 0, 0, 0); known
 * answer: counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8.  Normals, in fp64 from the outputs x0..x3 of counter q:
 * u_i = (x_i + 0.5) 2^-32, r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2), n_4q..4q+3 = r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3,
 * r1 sin 2 pi u3.  Colour noise: element e of the image's C H W values in NCHW order takes n_e; gray noise: pixel p of H W takes n_p in
 * every channel.  y = float(double(x) + double(sigma[b]) / 255 * n), rounded once; sigma[b] == 0 without flags returns x bit for bit.
 * DCPT_NOISE_CLIP clamps to [0, 1]; DCPT_NOISE_ROUND8 takes rint(255 v) / 255, half to even, after the clamp (with CLIP:
 * clamp(round(255 v), 0, 255) / 255 of add_gaussian_noise_pt); DCPT_NOISE_ONLY writes sigma / 255 * n instead of the sum.
 * An image's result depends on its own (x, sigma, key, gray) only, not on the batch around it or its position in it.  One launch, no
 * workspace, no atomics, no host synchronisation; the same input gives the same bits.
 * Errors (before the launch): null x (without DCPT_NOISE_ONLY), sigma, key or y, non-positive extents, C H W at or above 2^34 (the
 * counter's first word holds element / 4), a batch above 2^40 elements, unknown flag bits. */
#define DCPT_NOISE_CLIP 1     /* clamp to [0, 1] */
#define DCPT_NOISE_ROUND8 2   /* rint(255 v) / 255 */
#define DCPT_NOISE_ONLY 4     /* write the noise, not x + noise */
int dcpt_gauss_noise_fwd(const float* x, const float* sigma, const long long* key, const int* gray, float* y, int B, int C, int H, int W,
                         int flags, dcpt_stream_t stream);

/* ---- on-the-fly degradations: Poisson (shot) noise, on the device --------------------------------------------------
 * dcpt_poisson_noise_fwd replaces the Poisson family of basicsr/data/degradations.py:637-814 (generate_ / add_ / random_generate_ /
 * random_add_poisson_noise_pt): the per-image len(torch.unique(...)) loop (a sort and a host synchronisation per image) becomes the
 * population count of a 256-bit presence mask, torch.poisson a sampler by inversion on the Philox stream of dcpt_gauss_noise_fwd.  Two
 * launches for the batch, no sort, no read-back, no atomics; the same input gives the same bits, whatever the grid.
 *   x       dense NCHW fp32 [B][C][H][W]; always read (the rate depends on it), also with DCPT_NOISE_ONLY
 *   scale   fp32 [B] on the device: the factor on the noise of image b
 *   key     int64 [B] on the device: the Philox key of image b (words: its low and its high 32 bits)
 *   gray    int32 [B] on the device or null: non-zero gives image b noise made from its gray values, one plane shared by its channels
 *   y       dense NCHW fp32 [B][C][H][W]; y == x (in place) is allowed
 *   ws      dcpt_poisson_noise_ws_bytes(B, C, H, W) bytes (the query needs no device; 0 for an invalid shape).  On return (in stream order)
 *           its first B int32 hold vals[b]; the rest is scratch.
 * Per image b, with n = C H W and plane = H W:
 *   level(v) = (int) fmin(fmax(rint(255.0 * (double)v), 0.0), 255.0): half to even, NaN gives 0, so a level lies in 0..255.
 *   Colour image (gray null or gray[b] == 0): l_e = level(x_e) for every element e of the image, all channels.
 *   Gray image (gray[b] != 0; C must be 1 or 3): one value per pixel, g_p = x_p for C == 1 and (0.2989 R + 0.587 G) + 0.114 B for C == 3,
 *   in fp64 from the fp32 samples, each product and each sum rounded on its own; l_p = level(g_p).
 *   U = the number of distinct l of the image; vals = the smallest power of two >= U (U = 1 -> 1; at most 256).
 *   lambda = (double)(l * vals) / 255.0, one IEEE division of an exact integer; lambda <= 256.
 *   Uniforms: Philox4x32-10 as for dcpt_gauss_noise_fwd, key words the low / high half of key[b], counter (q, 0, 0, 0); its outputs x0..x3
 *   give u_j = (x_j + 0.5) 2^-32, and u_j belongs to element 4 q + j of the image (gray: to pixel 4 q + j, shared by the channels).
 *   Sampler: inversion by upward search in fp64, every product and sum rounded on its own (no fused multiply-add):
 *       p = exp(-lambda); s = p; k = 0;  while (s < u && k < 1023) { k += 1; p = (p * lambda) * R[k]; s = s + p; }
 *   with R[k] = 1.0 / k correctly rounded.  The cap 1023 only guards termination: for lambda <= 256 the sum passes the largest u,
 *   1 - 2^-33, long before it.
 *   Output, in fp64 and rounded once to fp32:  t = scale[b] * (k / vals - l / 255.0);  y = float((double)x + t).  Flags as for
 *   dcpt_gauss_noise_fwd: DCPT_NOISE_CLIP clamps to [0, 1], DCPT_NOISE_ROUND8 then takes rint(255 v) / 255, DCPT_NOISE_ONLY writes t.
 *   scale[b] == 0 without flags returns x bit for bit.
 * An image's result depends on its own (x, scale, key, gray) only.  In place works: the level pass has finished before the sampling kernel
 * starts, and a lane reads its own elements before it writes them.
 * Errors (before any launch): unknown flag bits; null x, scale, key, y or ws; a workspace below the query; non-positive extents, C H W at
 * or above 2^34, a batch above 2^40 elements; gray given with C other than 1 or 3. */
size_t dcpt_poisson_noise_ws_bytes(int B, int C, int H, int W);
int dcpt_poisson_noise_fwd(const float* x, const float* scale, const long long* key, const int* gray, float* y, void* ws, size_t ws_bytes,
                           int B, int C, int H, int W, int flags, dcpt_stream_t stream);

/* ---- on-the-fly degradations: synthetic blur, on the device -----------------------------------------------------
 * dcpt_filter2d_fwd replaces filter2D of basicsr/utils/img_process_util.py:7-31 (F.pad(mode="reflect") plus F.conv2d with B * C groups,
 * which materialises the padded batch and a weight repeated over the channels), the blur of USMSharp.forward (:73-82) with it.
 *   x      dense NCHW fp32 [B][C][H][W]
 *   kern   fp32 [B][K][K] when kern_per_image != 0, else [1][K][K] shared by the batch; every channel of an image uses its image's kernel
 *   y      dense NCHW fp32 [B][C][H][W]; must not overlap x (an output reads its neighbours' pixels)
 * A correlation, no flip, as F.conv2d, over the image reflect-padded by r = K / 2: index -i reads i and H - 1 + i reads H - 1 - i (the edge
 * sample is not repeated):
 *     y[b][c][i][j] = sum over dy, dx in 0 .. K - 1 of kern[b][dy][dx] * xpad[b][c][i + dy][j + dx],  xpad[p][q] = x[refl(p - r)][refl(q - r)]
 * Arithmetic, per output: acc = 0.0 (double); for dy = 0 .. K - 1 (outer), for dx = 0 .. K - 1 (inner), both ascending:
 *     acc = fma((double)kern[b][dy][dx], (double)xpad[..], acc);     y = (float)acc, the one fp32 rounding.
 * The product of two fp32 values is exact in fp64, so a step rounds once whether it is a fused multiply-add or a multiply and an add, and
 * the sum has ONE value: a host loop of plain float64 multiply-adds in that order (basicsr.data.filter2d_host) gives the same bits.  The
 * sum is not split over lanes, rows or partial accumulators.
 * One launch, no workspace, no atomics, no host synchronisation; the same input gives the same bits.
 * Errors (before the launch): null pointers; B, C, H or W below 1; K even, below 1 or above 51; K / 2 >= H or K / 2 >= W (torch's reflect
 * padding refuses it too); y overlapping x; more than 2^31 - 1 tiles of 32 x 64 in the batch. */
int dcpt_filter2d_fwd(const float* x, const float* kern, float* y, int B, int C, int H, int W, int K, int kern_per_image,
                      dcpt_stream_t stream);

/* ---- on-the-fly degradations: the resize of the second-order chain, on the device ---------------------------------
 * dcpt_interp_fwd replaces F.interpolate(mode = "area" | "bilinear" | "bicubic", align_corners=False, no antialiasing) as the reference's
 * Real-ESRGAN degradation chain calls it.  (dcpt_imresize_fwd is another arithmetic: MATLAB bicubic with antialiasing from host tables.)
 *   x        dense NCHW fp32 [B][C][H][W]
 *   y        dense NCHW fp32 [B][C][Ho][Wo]; must not overlap x
 *   mode     DCPT_INTERP_AREA, DCPT_INTERP_BILINEAR or DCPT_INTERP_BICUBIC
 *   ratio_h, ratio_w   source pixels per destination pixel.  torch uses 1 / scale_factor when a scale factor is given and H / Ho when a
 *            size is given; the caller passes whichever applies.  Not used by the area mode.
 * The taps of output index d of one axis (n source samples, m destination samples, ratio r); source coordinates in fp64, each product and
 * sum rounded on its own:
 *   area (adaptive_avg_pool2d): s = floor(d n / m), e = ceil((d + 1) n / m) in integers; taps s .. e - 1, each weighted 1.0 / (e - s).
 *   bilinear: src = max((d + 0.5) r - 0.5, 0); i0 = min(floor(src), n - 1); t = src - i0; i1 = min(i0 + 1, n - 1); taps i0, i1 with the
 *       weights 1 - t, t.
 *   bicubic (A = -0.75): src = (d + 0.5) r - 0.5, not clamped; i0 = floor(src); t = src - i0; taps clamp(i0 - 1 + k, 0, n - 1), k = 0 .. 3,
 *       with the weights c2(t + 1), c1(t), c1(1 - t), c2(2 - t);  c1(v) = ((A + 2) v - (A + 3)) v v + 1,
 *       c2(v) = ((A v - 5 A) v + 8 A) v - 4 A.
 * Arithmetic, per output (i, j), with the row taps (ia, wh[a]) of i and the column taps (jb, ww[b]) of j, in fp64:
 *     acc = 0;  for a ascending: { inner = 0;  for b ascending: inner = fma(ww[b], (double)x[ia][jb], inner);  acc = fma(wh[a], inner, acc); }
 * DCPT_INTERP_CLIP clamps acc to [0, 1]; DCPT_INTERP_ROUND8 then takes rint(255 v) / 255, half to even (as DCPT_NOISE_*);
 * y = (float)acc, the one fp32 rounding.  An output of equal size (ratio 1) returns x.
 * One launch, no workspace, no atomics, no host synchronisation; the same input gives the same bits.  The taps of an output tile are
 * computed once per workgroup and shared by the image's channels; the source is read through the caches, not staged (resize.hip says why).
 * Errors (before the launch): null pointers; non-positive extents; an unknown mode or flag bit; a source or destination plane above 2^30
 * pixels; a batch above 2^40 elements; for bilinear and bicubic a ratio that is not in (0, 2^30] (a NaN included); y overlapping x. */
#define DCPT_INTERP_AREA 0
#define DCPT_INTERP_BILINEAR 1
#define DCPT_INTERP_BICUBIC 2
#define DCPT_INTERP_CLIP 1     /* clamp to [0, 1] */
#define DCPT_INTERP_ROUND8 2   /* rint(255 v) / 255 */
int dcpt_interp_fwd(const float* x, float* y, int B, int C, int H, int W, int Ho, int Wo, int mode, double ratio_h, double ratio_w, int flags,
                    dcpt_stream_t stream);

/* ---- the kNN degradation probe: fp64 distances and the neighbour vote, on the device ------------------------------
 * replaces what the reference's knn.py leaves to scikit-learn on the host (KNeighborsClassifier(5).fit / predict over the flattened decoder
 * features of knn_gen.py): the distances between a few hundred rows of 10^5 .. 10^6 numbers each, and the majority vote.
 *
 * dcpt_pdist2_fwd: d2[i][j] = the squared Euclidean distance between row i of xq and row j of xt.
 *   xq     [Nq] rows of D elements, row i at element i ldq; fp32, or bf16 with DCPT_PDIST_BF16 (both operands)
 *   xt     [Nt] rows of D elements, row j at element j ldt; xq == xt is allowed
 *   d2     fp64 [Nq] rows of Nt, row i at element i ldd
 * Arithmetic: every element is converted to fp64 (exact).  G_ij = sum_k q_ik t_jk, n_i = sum_k q_ik^2, m_j = sum_k t_jk^2; each product of
 * two fp32 or bf16 values is exact in fp64, the sums are fp64 in an order the kernel fixes (the k-range in `ksplit` chunks, a chunk's sum
 * in ascending k on the fp64 matrix cores for G and over 256 interleaved lanes and a fixed tree for n and m, the chunks added in chunk order).
 *     d2[i][j] = max(0, (n_i + m_j) - 2 G_ij)          (a NaN stays a NaN)
 * ksplit: the number of chunks of the k-range, chunk c = columns [c L, min(D, (c + 1) L)) with L = 4 ceil(ceil(D / 4) / ksplit); 0: the
 * library chooses from the shape (about 1024 workgroups of 64 x 64 tiles, chunks of at least 512 columns), a positive value forces it.
 * Partial tiles and norms go to the workspace with plain stores and a second pass adds them: no atomics.
 * Contract: d2[i][j] depends only on row i of xq, row j of xt, D, the element type and the effective ksplit -- not on i, j, Nq, Nt, the
 * leading dimensions or the other rows.  So two runs give the same bits, permuting the rows of xt permutes the columns of d2 bit for bit,
 * and duplicate rows get equal distances.  (Not promised: a zero diagonal or bitwise symmetry for xq == xt.)
 * dcpt_pdist2_ws_bytes needs no device and returns 0 for a refused shape.  Four launches, no host synchronisation.
 * Errors (before any launch): unknown flag bits; null pointers; Nq, Nt or D below 1; Nq or Nt above 65535; ldq or ldt below D, ldd below
 * Nt; ksplit below 0, above ceil(D / 4) or above 65535; a workspace below the query.
 *
 * dcpt_knn_vote_fwd: the k nearest training columns of every query row of d2 and their majority label, for S splits in one launch.
 *   d2       fp64, row r at element r ldd
 *   q_idx    int32 [S][nq], t_idx int32 [S][nt]: the rows and the columns of d2 that split s uses (device memory; not checked)
 *   labels   int32, labels[c] the label of column c of d2 (any value)
 *   nbr      int32 [S][nq][k]: positions in the split's t_idx, nearest first;  nbr_d2 fp64 [S][nq][k]: their distances;  pred int32 [S][nq]
 * Neighbours are ordered by (distance, position in t_idx) ascending -- a stable sort: equal distances go to the lower position, -0 equals
 * +0 -- and a NaN distance ranks after every number.  The predicted label has the largest count among the k neighbours; on equal counts
 * the smallest label value wins (scikit-learn's uniform-weight vote).  One wave per (query, split), one launch, no workspace.
 * Errors (before the launch): null pointers; S, nq or nt below 1; k below 1, above 32 or above nt; ldd below 1. */
#define DCPT_PDIST_BF16 1   /* rows are bf16 instead of fp32 (the taps of a bf16-storage encoder) */
size_t dcpt_pdist2_ws_bytes(int Nq, int Nt, long long D, int ksplit);
int dcpt_pdist2_fwd(const void* xq, const void* xt, double* d2, void* ws, size_t ws_bytes, int Nq, int Nt, long long D, long long ldq,
                    long long ldt, long long ldd, int ksplit, int flags, dcpt_stream_t stream);
int dcpt_knn_vote_fwd(const double* d2, long long ldd, const int* q_idx, const int* t_idx, const int* labels, int S, int nq, int nt, int k,
                      int* nbr, double* nbr_d2, int* pred, dcpt_stream_t stream);

/* ---- exact t-SNE of the probe's features, on the device -------------------------------------------------------------
 * the other half of the reference's feature analysis (t_sne.py: sklearn.manifold.TSNE(n_components=2) on the unit-length rows): the rules
 * of scikit-learn's method="exact", as functions of the squared-distance matrix dcpt_pdist2_fwd produces.  All arithmetic is fp64; plain
 * launches, plain stores, no atomics; two runs give the same bits; a row's result depends on that row's inputs and on N only.
 * EPS = 2^-52.  Every sum is taken in one of two orders: BLOCK order -- lane t of 256 adds its terms j = t, t + 256, ... in ascending j,
 * the 256 sums go through a fixed binary tree (t += t + 128, 64, ... 1) -- or WAVE order -- lane t of 64 adds j = t, t + 64, ..., the 64
 * sums go through the xor butterfly 32, 16, ... 1.  N is 2 .. 65535 everywhere and only two output dimensions exist.
 *
 * dcpt_tsne_affinity_fwd: d2 fp64 [N] rows of N, row i at element i ldd -> pcond fp64 (row i at i ldp), beta fp64 [N], steps int32 [N].
 * Per row i, j over all columns but i (the diagonal of d2 is never read; pcond[i][i] = 0):
 *     beta = 1; lo = -inf; hi = +inf
 *     for l in 0..99:
 *         p_j = exp(-d2[i][j] * beta);  s = sum_j p_j (block order);  if s == 0: s = 1e-8;  p_j = p_j / s
 *         sd = sum_j d2[i][j] * p_j (block order);  e = log(s) + beta * sd - log(perplexity);  if |e| <= 1e-5: break
 *         e > 0: lo = beta; beta = beta * 2 if hi == +inf else (beta + hi) / 2
 *         else:  hi = beta; beta = beta / 2 if lo == -inf else (beta + lo) / 2
 * pcond holds the p of the last step run, steps the index l of that step (99 when the search did not end), beta the value after the loop.
 * scikit-learn rounds the distances to float32 before this search; the kernel does not.  beta moves by exact dyadic arithmetic.
 * Errors: null pointers, N outside 2 .. 65535, a perplexity that is not finite or outside [1, N), ldd or ldp below N, pcond == d2.
 *
 * dcpt_tsne_joint_fwd: r_i = sum_{j != i} (pcond_ij + pcond_ji) (block order), S = max(sum_i r_i, EPS) (block order over i),
 *     P_ij = P_ji = max((pcond_ij + pcond_ji) / S, EPS) for i != j, P_ii = 0.     P (row i at i ldo) may be pcond; P is symmetric bit for bit.
 * ws: dcpt_tsne_steps_ws_bytes(N).  Errors: null pointers, N, ldp or ldo below N, P == pcond with ldo != ldp, a short workspace.
 *
 * dcpt_tsne_steps_fwd: n_steps >= 0 descent iterations on Y, update and gains (fp64 [N][2] each, dense), in place.  One iteration, with
 * P' = exaggeration P and w_ij = 1 / (1 + (dx^2 + dy^2)), (dx, dy) = y_i - y_j, an IEEE division:
 *     z_i = sum_{j != i} w_ij (wave order);  Z = sum_i z_i (wave order over i);  Q_ij = max(w_ij / Z, EPS)
 *     g_i = 4 * sum_{j != i} (P'_ij - Q_ij) w_ij (y_i - y_j)      (wave order, per component)
 *     per component: gains = (update * g < 0) ? gains + 0.2 : gains * 0.8;  gains = max(gains, min_gain);  g = g * gains;
 *                    update = momentum * update - lr * g;  y = y + update
 * On the last of the n_steps iterations also (device array stats[2]; nothing is read back):
 *     stats[0] = sum_i [ sum_{j != i} P'_ij log(max(P'_ij, EPS) / Q_ij) (wave order) ] (block order over i)    -- at the Y before that move
 *     stats[1] = sqrt( sum_i (g_i0^2 + g_i1^2) (block order over i) ) of the gain-scaled g: scikit-learn's gradient norm
 * n_steps = 0 touches nothing.  Two launches per iteration, a third on the last; the new points go to a second embedding buffer in the
 * workspace, so no wave reads a row that another writes.  out_dims must be 2.
 * dcpt_tsne_kl_fwd: the same evaluation at a Y that does not move: grad fp64 [N][2] = the plain g, stats[0] as above, stats[1] = |g|.
 * dcpt_tsne_steps_ws_bytes needs no device; it returns 0 for N outside 2 .. 65535 and serves the joint pass, the steps and the KL pass.
 * Errors (before any launch): null pointers, out_dims other than 2, N outside 2 .. 65535, ldp below N, n_steps below 0, a parameter that
 * is not finite, a Y that is not 16-byte aligned, a workspace below the query. */
size_t dcpt_tsne_steps_ws_bytes(int N);
int dcpt_tsne_affinity_fwd(const double* d2, long long ldd, double* pcond, long long ldp, double* beta, int* steps, int N,
                           double perplexity, dcpt_stream_t stream);
int dcpt_tsne_joint_fwd(const double* pcond, long long ldp, double* P, long long ldo, void* ws, size_t ws_bytes, int N,
                        dcpt_stream_t stream);
int dcpt_tsne_steps_fwd(const double* P, long long ldp, double* Y, double* update, double* gains, double* stats, void* ws,
                        size_t ws_bytes, int N, int out_dims, int n_steps, double exaggeration, double momentum, double lr,
                        double min_gain, dcpt_stream_t stream);
int dcpt_tsne_kl_fwd(const double* P, long long ldp, const double* Y, double* grad, double* stats, void* ws, size_t ws_bytes, int N,
                     int out_dims, double exaggeration, dcpt_stream_t stream);

/* ---- optional launch profiling (bench.py) -------------------------------------------------------
 * While enabled, MFMA GEMM launches are bracketed by HIP events on their own stream: every launch for on = 1, every
 * on-th launch for on > 1 (sampling keeps the perturbation of a timed region small: an event pair costs ~3 us of queue time).
 * dcpt_prof_read waits for them and writes rows of 8 doubles {class id, M, N, K, launches, total ms,
 * algorithmic flops, algorithmic bytes}, one per (class, shape); class id = 16*loaderA + epilogue (NT) or
 * 512 + 8*loaderX + loaderY (TN); 1024 + i for a few non-GEMM launches (1032 / 1033: the level pass and the sampler of
 * dcpt_poisson_noise_fwd, M = the batch's elements; 1034 .. 1036: the norm, MFMA and finishing passes of dcpt_pdist2_fwd; 1037:
 * dcpt_knn_vote_fwd; 1038 .. 1042: the affinity, joint, z-partial, gradient and statistics launches of dcpt_tsne_*_fwd, M = N). */
int dcpt_prof_enable(int on);
int dcpt_prof_read(double* out, int max_rows);

/* ---- weight-gradient side stream ------------------------------------------------------------------
 * dcpt_nafblock_bwd enqueues its four weight-gradient GEMMs (+ slab reductions) on an internal low-priority
 * HIP stream, forked from and joined back into `stream` with events inside the call (callers see ordinary
 * stream semantics).  on = 0 keeps everything on the caller's stream (also: DCPT_SIDE_STREAM=0 in the
 * environment, and automatically while `stream` is being captured into a graph).  Returns the previous setting. */
int dcpt_set_side_stream(int on);

/* ---- optimizer step --------------------------------------------------------------------------------------
 * AdamW (decoupled weight decay) over a LIST of fp32 tensors, the update that closes every training step of the path: replaces
 * torch.optim.AdamW(...).step() as built by basicsr/models/base_model.py:70-93 and called by sr_model.py:118 and
 * degradation_classification_pretrain_model.py:170-173.  Per element, in fp32 and in the order of torch's fused kernel:
 *     p -= lr wd p;  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g g;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * `params / grads / exp_avg / exp_avg_sq / numel` are HOST arrays of n entries (device pointers and element counts, tensor i dense in
 * any layout shared by its four buffers; entries with numel 0 are skipped); bias_correction{1,2} = 1 - beta{1,2}^step for the step
 * being taken (step >= 1).  maximize != 0 negates the gradients.  A few launches on `stream` for any n (80 tensors per launch, the
 * pointers travel as kernel arguments: nothing is copied or allocated). */
typedef struct {
    double lr, beta1, beta2, eps, weight_decay;   /* doubles as the host holds them: 1 - beta is formed in double (1 - 0.999 in fp32 is off by 1e-5) */
    double bias_correction1, bias_correction2;
    int maximize;
} dcpt_adamw_hparams;
int dcpt_adamw_step(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    const int64_t* numel, const dcpt_adamw_hparams* h, dcpt_stream_t stream);

/* ---- fused step tail: gradient-norm clip and EMA around the AdamW kernel ---------------------------------------
 * replaces the three calls that end a fine-tuning step of the reference, sr_model.py:166-174 (clip_grad_norm_(parameters, max_norm),
 * optimizer.step(), model_ema(decay)) with base_model.py:86-95 (model_ema: ema = decay ema + (1 - decay) p per parameter).
 *
 * dcpt_grad_norm: the global 2-norm of a LIST of fp32 gradients and torch's clip coefficient, both left in DEVICE memory:
 *     out2[0] = norm = (float)sqrt(sum g^2), the squares accumulated in fp64 (one double per 4096-element block in `workspace`, summed
 *     in a fixed order: two calls on the same data give the same bits);  out2[1] = coef = min(1, max_norm / (norm + 1e-6)) in fp32, a
 *     NaN norm giving a NaN coefficient (clip_grad_norm_ with error_if_nonfinite=False).
 * `grads / numel` are HOST arrays of n entries (0 <= numel < 2^32 - 4096; empty entries are skipped and may be null).  `workspace` holds
 * dcpt_grad_norm_ws_bytes(n, numel) bytes = 8 x sum ceil(numel / 4096) (the query needs no device; 0 for an invalid list).  One launch
 * per 80 non-empty tensors and one single-block launch that writes out2 -- also when every tensor is empty ({0, 1}).  Arguments are
 * checked before the first launch.
 *
 * dcpt_adamw_step_ex: dcpt_adamw_step with two optional stages in the same kernel.  clip_coef != NULL: a DEVICE pointer to one float
 * (out2 + 1 of dcpt_grad_norm), g *= *clip_coef before the update -- the gradient buffers themselves are NOT scaled.  ema != NULL: a
 * HOST array of n device pointers, tensor i laid out as params[i]; after the update ema[i] = ema[i] ema_decay + (1 - ema_decay) p_new
 * (the product rounded, then one fused multiply-add: the rounding of torch's _foreach_mul_ / _foreach_add_(alpha) pair).  With both
 * NULL it is dcpt_adamw_step. */
size_t dcpt_grad_norm_ws_bytes(int n, const int64_t* numel);
int dcpt_grad_norm(int n, const float* const* grads, const int64_t* numel, float max_norm, void* workspace, size_t workspace_bytes,
                   float* out2, dcpt_stream_t stream);
int dcpt_adamw_step_ex(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       float* const* ema, const int64_t* numel, const dcpt_adamw_hparams* h, const float* clip_coef, double ema_decay,
                       dcpt_stream_t stream);

/* ---- gradient all-reduce (data-parallel step) -------------------------------------------------------
 * replaces what torch DistributedDataParallel does for the reference (basicsr/models/base_model.py:108-115: bucketed
 * all-reduce(SUM) / world of the gradients; :448 the loss reduce) for hosts that drive the collective themselves:
 * in-place `ncclAllReduce(SUM, fp32)` of buf[0..n) over the CALLER-PROVIDED RCCL communicator (an ncclComm_t created by the
 * launcher, one rank per GPU), enqueued on `stream`, followed by buf *= scale (pass 1/world for the mean, 1 to skip).
 * The library does not create communicators or bootstrap ranks, and it does not link RCCL: the entry point is resolved on
 * first use from the copy already loaded in the process (torch's) or the system's librccl.so.1.  Overlap with backward
 * is the caller's choice of stream (a side stream + events, as DDP's bucket hooks do).
 * basicsr/ in this repository keeps the reference's own mechanism (torch DDP over backend "nccl" = RCCL) for the training
 * step; this entry point is the C-ABI form of the same collective (SURVEY 8b minimum export set). */
int dcpt_allreduce_flat(float* buf, size_t n, void* rccl_comm, float scale, dcpt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DCPT_HIP_H */
