// Internal launchers for the non-GEMM kernels (all NHWC fp32; every launcher enqueues on `s`,
// never synchronises, returns DCPT_OK or sets the error string).
#pragma once
#include "dcpt_common.h"

// ---- ln.hip -------------------------------------------------------------------------------
int launch_ln_stats(const float* x, float* mu, float* rstd, int64_t M, int C, float eps, hipStream_t s);
int launch_ln_fwd(const float* x, const float* w, const float* b, float* y, float* mu, float* rstd, int64_t M, int C,
                  float eps, hipStream_t s);
// y = [relu]( LN(x)*w + b [+ res] )   (channels-first LayerNorm of the classifier head, fused tail)
int launch_ln_act_fwd(const float* x, const float* w, const float* b, const float* res, int relu, float* y, float* mu,
                      float* rstd, int64_t M, int C, float eps, hipStream_t s);
// as launch_ln_bwd, with the incoming gradient first masked by (ymask > 0) and optionally copied to gmasked
int launch_ln_act_bwd(const float* gy, const float* x, const float* mu, const float* rstd, const float* w, const float* dres,
                      const float* ymask, float* gmasked, float* dx, float* part, int nblk, int64_t M, int C, hipStream_t s);
// general form: biasfree = 1 selects Restormer's BiasFree_LayerNorm backward (part row 1 is then meaningless)
int launch_ln_bwd_ex(const float* gy, const float* x, const float* mu, const float* rstd, const float* w, const float* dres,
                     const float* ymask, float* gmasked, int biasfree, float* dx, float* part, int nblk, int64_t M, int C,
                     hipStream_t s);
// dx = LN-backward(gy; x, mu, rstd, w) (+ dres if non-null).  Column sums go to part[nblk][3][C]
// (0: sum gy*xhat, 1: sum gy, 2: sum dx_total); returns nblk through *nblk_out.
int ln_bwd_num_blocks(int64_t M, int C);
int launch_ln_bwd(const float* gy, const float* x, const float* mu, const float* rstd, const float* w, const float* dres,
                  float* dx, float* part, int nblk, int64_t M, int C, hipStream_t s);
// out[j][c] = sum_r part[r][j][c], j < nj  (deterministic order); out rows may be null to skip
int launch_colpart_reduce(const float* part, int R, int nj, int C, float* out0, float* out1, float* out2, hipStream_t s);

// ---- dwconv.hip ---------------------------------------------------------------------------
struct DwGeom {
    int B, H, W, C;  // C = gated channels (t1 has 2C)
};
int dw_num_blocks_per_image(const DwGeom& g);            // NBLK for fwd / bwd_a (quads of C)
int launch_dw_pack_weights(const float* w2, float* w2p, int C2, hipStream_t s);  // [C2][9] -> [9][C2]
// t2 = SG(dw3x3(t1) + b2); pool_part[B][NBLK][C] partial sums of t2
int launch_dw_fwd(const float* t1, const float* w2p, const float* b2, float* t2, float* pool_part, const DwGeom& g,
                  hipStream_t s);
// dw2[ch*9+tap] and db2[ch] from wpart[R][10][C2]
int launch_dw_wgrad_reduce(const float* wpart, int R, int C2, float* dw2, float* db2, hipStream_t s);

// dwring.hip: the same forward on an LDS-DMA row ring (fp32 / bf16 storage); pool_part[B][dw_ring_num_blocks_per_image][C]
bool dw_ring_usable(const DwGeom& g, int elem_bytes);
int dw_ring_num_blocks_per_image(const DwGeom& g, int elem_bytes);
int launch_dw_ring_fwd_f32(const float* t1, const float* w2p, const float* b2, float* t2, float* pool_part, const DwGeom& g, hipStream_t s);
// SimpleGate-backward + transposed depthwise + tap-gradient partials in one pass (da = gate-backward(dts * s + dpool) is never
// written): dt1 and wpart[B][dw_ring_bwd_num_blocks_per_image][10][2C]
bool dw_ring_bwd_usable(const DwGeom& g, int elem_bytes);
int dw_ring_bwd_num_blocks_per_image(const DwGeom& g);
int launch_dw_ring_bwd_fused_f32(const float* dts, const float* t1, const float* w2p, const float* b2, const float* simg, const float* dpool,
                                 float* dt1, float* wpart, const DwGeom& g, hipStream_t s);
// Restormer forms on the same ring kernel: the GDFN gate gelu(a_1) a_2 backward (launch_dw_gelu_bwd_a + launch_dw_generic_bwd in one
// pass, da never written) and the plain depthwise backward; block counts from dw_ring_bwd_num_blocks_per_image({B, H, W, Ch | Ctot / 2})
int launch_dw_ring_gelu_fwd_f32(const float* u, const float* w2p, float* t, int B, int H, int W, int Ch, hipStream_t s);
// tout != null: also writes the gate product gelu(a_1) a_2 [M][Ch] (bit-identical to launch_dw_ring_gelu_fwd_f32) for callers that did not keep it
int launch_dw_ring_bwd_gelu_f32(const float* dt, const float* u, const float* w2p, float* du, float* wpart, int B, int H, int W, int Ch, hipStream_t s,
                                float* tout = nullptr);
int launch_dw_ring_bwd_plain_f32(const float* dy, const float* x, const float* w2p, float* dx, float* wpart, int B, int H, int W, int Ctot, hipStream_t s);

// generic depthwise pieces (Restormer): w2p is the [9][Ctot] packed weight (launch_dw_pack_weights)
int dw_num_blocks_generic(int B, int H, int W, int Ctot);
// t[M][Ch] = gelu(dw(u)[:, :Ch]) * dw(u)[:, Ch:]   (u has 2*Ch channels, no bias)
int launch_dw_gelu_fwd(const float* u, const float* w2p, float* t, int B, int H, int W, int Ch, hipStream_t s);
int launch_dw_gelu_bwd_a(const float* dt, const float* u, const float* w2p, float* da, int B, int H, int W, int Ch, hipStream_t s);
// y = dw(x) over Ctot channels; sq_part[B][nblk][nsq] partial sums of y^2 for the first nsq channels (may be null)
int launch_dw_plain_fwd(const float* x, const float* w2p, float* y, float* sq_part, int nsq, int B, int H, int W, int Ctot,
                        hipStream_t s);
// dx = dw^T(dy); wpart[B*nblk][10][Ctot] partials of the tap gradients (rows 0..8) -- reduce with launch_dw_wgrad_reduce
int launch_dw_generic_bwd(const float* dy, const float* x, const float* w2p, float* dx, float* wpart, int B, int H, int W, int Ctot,
                          hipStream_t s);

// ---- misc.hip -----------------------------------------------------------------------------
// pooled[b][k] = (sum_blk pool_part[b][blk][k]) / P ;  s[b][n] = sum_k Wsca[n][k]*pooled[b][k] + bsca[n]
int launch_sca_fwd(const float* pool_part, int nblk, const float* Wsca, const float* bsca, float* pooled, float* simg,
                   int B, int C, int P, hipStream_t s);
// ds[b][k] = sum_{m in image b} dts[m][k] * t2[m][k]   (two-stage, deterministic)
int sca_ds_num_blocks(int P);
int sca_ds_fused_slices(int P);   // P / 128 when the E_DOTCOL form applies, else 0
// backward: part[b][j][k] = sum over the j-th pixel slice of image b of dts*t2  (j < sca_ds_num_blocks(P))
int launch_sca_ds_part(const float* dts, const float* t2, float* ds_part, int B, int C, int P, hipStream_t s);
// (the slices may also come out of the dts GEMM's E_DOTCOL epilogue: 128-pixel slices, nslices = P / 128)
// critical path: dpool[b][k] = (1/P) sum_n Wsca[n][k] * sum_j part[b][j][n]
// (ds_out != null: also stores ds[b][n] = sum_j part[b][j][n], which the parameter-gradient side needs)
int launch_sca_dpool(const float* ds_part, int nslices, const float* Wsca, float* dpool, int B, int C, int P, hipStream_t s, float* ds_out = nullptr);
// parameter gradients (off the critical path): ds = sum_j part, dWsca = ds^T pooled, dbsca = sum_b ds
int launch_sca_wgrad(const float* ds_part, int nslices, float* ds, const float* pooled, float* dWsca, float* dbsca, int B, int C,
                     hipStream_t s);
// dpool[b][k] = (sum_n Wsca[n][k]*ds[b][n]) / P ; dWsca[n][k] = sum_b ds[b][n]*pooled[b][k] ; dbsca[n] = sum_b ds[b][n]

// TLSC box mean (arch_util.py:378-396): out[M][C] local k1 x k2 mean of in, replicate-padded; rowsum: [B][H][W-k2+1][C] scratch
int launch_box_mean(const float* in, float* rowsum, float* out, int B, int H, int W, int C, int k1, int k2, hipStream_t s);
// rcan.hip: RCAN's channel attention of B images from the per-(128-row tile, image) column sums of t (E_BIASCOL / EB_BIASCOL): pooled, s [B][C]
int launch_rcan_ca_fwd(const float* colpart, const float* w1, const float* b1, const float* w2, const float* b2, float* pooled, float* sc, int B,
                       int P, int C, int Cr, hipStream_t s);

enum WPackMode {
    WP_TRANSPOSE = 0,   // out[k][n] = in[n][k] * (rs ? rs[n] : 1)             in: [N][K]
    WP_DOWN = 1,        // out[oc][ij*C + ic] = in[oc][ic][ij]                  in: [N=2C][C][2][2]  (K = 4C)
    WP_DOWN_T = 2,      // out[ij*C + ic][oc] = in[oc][ic][ij]
    WP_UP = 3,          // out[ij*G + kk][ic] = in[4kk+ij][ic]                  in: [N=4G][K]
    WP_UP_T = 4,        // out[ic][ij*G + kk] = in[4kk+ij][ic]
    WP_CONV3 = 5,       // out[oc][tap*Ci + ic] = in[oc][ic][tap]              in: [N=Co][Ci][3][3]  (K = 9*Ci)
    WP_CONV3_T = 6      // out[ic][tap*Co + oc] = in[oc][ic][8-tap]            (dgrad: N' = Ci rows, K' = 9*Co)
};
int launch_wpack(const float* in, float* out, const float* rs, int N, int K, int mode, hipStream_t s);
// up to WPACK_MAX_JOBS WP_TRANSPOSE jobs (out[k][n] = in[n][k] * rs[n]) in one launch
constexpr int WPACK_MAX_JOBS = 6;
struct WpackJobs {
    const float* in[WPACK_MAX_JOBS];
    float* out[WPACK_MAX_JOBS];
    const float* rs[WPACK_MAX_JOBS];
    int N[WPACK_MAX_JOBS], K[WPACK_MAX_JOBS];
    int n;
};
int launch_wpack_multi(const WpackJobs& jobs, hipStream_t s);

enum WReduceMode { WR_PLAIN = 0, WR_DOWN = 1, WR_UP = 2, WR_CONV3 = 3 };
// dW = rowscale[n] * sum_s slab[s][n][k] (layout per mode)
// optional: dgain[n] = sum_k W[n][k]*G[n][k] + wbias[n]*cs[n];  dbias[n] = rowscale[n]*cs[n]
//           (cs = sum over the cs_rows partial rows colsum[r][n])
int launch_wgrad_reduce(const float* slab, const float* colsum, int splits, int cs_rows, int N, int K, const float* rowscale,
                        const float* W, const float* wbias, float* dW, float* dgain, float* dbias, int mode, hipStream_t s);
// The fp32 weight gradient of a layer on rows, start to end: plans the split of the TN GEMM, runs it into slab / colsum and reduces:
//   dW[n][k] = sum_m X[m][n] Y'(m, k)   (mode WR_PLAIN, or WR_CONV3: dW[n][ic][tap] from Y' = the 3x3 im2col),  db[n] = sum_m X[m][n]
// proto carries the Y loader's fields (LayerNorm / scale pointers, conv geometry gH, gW, gC); colsum == null: no bias gradient.
// A layer whose output is scaled by a learnt per-channel gain (NAFBlock's beta / gamma) passes WgradGain: dW is then scaled by
// rowscale[n], db too, and dgain[n] = sum_k W[n][k] G[n][k] + wbias[n] db'[n].
// wgrad_need raises *slab_floats / *colsum_floats to what one such gradient needs, so a layout calls it once per layer that shares the buffers.
struct GemmTN;
struct WgradGain {
    const float *rowscale, *W, *wbias;
    float* dgain;
};
void wgrad_need(int64_t M, int N, int K, size_t* slab_floats, size_t* colsum_floats);
int launch_wgrad(const GemmTN& proto, int yload, const float* X, int ldx, int N, const float* Y, int ldy, int K, int64_t M, float* slab,
                 float* colsum, float* dW, float* db, int mode, hipStream_t s, const WgradGain& gain = WgradGain{});
// The backward of a biased dense 3x3 conv on NHWC rows, y = conv3x3(x; w [Cout][Cin][3][3]) + b, from dz = dL/dy [M][Cout]:
// packs w transposed with flipped taps into wT [Cin][9 Cout], dx [M][Cin] = epi(conv3x3(dz; wT)) with the GEMM epilogue epi and its
// res / slope operands (E_PLAIN; E_RESID adds res; E_RELU / E_LRELU mask by the saved activation res), then dw, db from dz and x.
int launch_conv3_bwd(const float* dz, const float* x, const float* w, float* wT, int B, int H, int W, int Cin, int Cout, int epi,
                     const float* res, float slope, float* dx, float* slab, float* colsum, float* dw, float* db, hipStream_t s);
// as launch_wgrad_reduce, with slab s weighted by kscale[(s / splits_per_image)][k] (every split inside one image; SCA scale folded into the reduce)
int launch_wgrad_reduce_scaled(const float* slab, const float* colsum, int splits, int cs_rows, int N, int K, const float* rowscale,
                               const float* W, const float* wbias, float* dW, float* dgain, float* dbias, int mode,
                               const float* kscale, int splits_per_image, hipStream_t s);

// ---- conv3x3.hip ----------------------------------------------------------------------------
// small (NCHW, Cs <= 4) -> big (NHWC, Cb % 4 == 0):  y[p][c] = sum_{s,tap} x[p+off(tap)][s] * W(c,s,tap) (+ bias[c])
//   wmode 0: W(c,s,tap) = w[(c*Cs+s)*9+tap]      (forward of a Cs->Cb conv, weight [Cb][Cs][3][3])
//   wmode 1: W(c,s,tap) = w[(s*Cb+c)*9+(8-tap)]  (dgrad of a Cb->Cs conv, weight [Cs][Cb][3][3])
int launch_conv3x3_s2b(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cs, int Cb,
                       int wmode, hipStream_t s);
// big (NHWC) -> small (NCHW): y[p][s] = sum_{c,tap} x[p+off(tap)][c] * W(s,c,tap) (+ bias[s]) (+ res[p][s])
//   wmode 0: W(s,c,tap) = w[(s*Cb+c)*9+tap]      (forward of a Cb->Cs conv)
//   wmode 1: W(s,c,tap) = w[(c*Cs+s)*9+(8-tap)]  (dgrad of a Cs->Cb conv)
int launch_conv3x3_b2s(const float* x, const float* w, const float* bias, const float* res, float* y, int B, int H, int W,
                       int Cs, int Cb, int wmode, hipStream_t s);
// G[c][s][tap] = sum_p big[p][c] * small[p+off(tap)][s];  bsum[c] = sum_p big[p][c]
//   omode 0: dW[(c*Cs+s)*9+tap] = G      omode 1: dW[(s*Cb+c)*9+(8-tap)] = G
int conv3x3_wgrad_num_blocks(int B, int H, int W, int Cb);
int launch_conv3x3_wgrad(const float* big, const float* small, float* part, int nblk, float* dW, float* bsum, int B, int H,
                         int W, int Cs, int Cb, int omode, hipStream_t s);
// out[c] = sum_{b,h,w} x[b][c][h][w]   (NCHW, tiny C); part: [C][128] scratch
int launch_nchw_channel_sum(const float* x, float* part, float* out, int B, int C, int HW, hipStream_t s);

// restormer.hip: fp32 pieces of the MDTA / GDFN blocks shared with their bf16-storage form (restormer_bf16.hip)
int launch_mdta_sq_norm(const float* part, int nblk, float* nrm, int B, int C2, hipStream_t s);
int launch_mdta_attn_finalize(const float* slab, int splits, const float* nrm, const float* temp, float* ghat, float* attn, float* attnT,
                              int B, int heads, int ch, int c, bool softmax, hipStream_t s);
int launch_mdta_attn_bwd(const float* slab, int splits, const float* attn, const float* ghat, const float* nrm, const float* temp, float* dG,
                         float* dGT, float* cqk, float* dtemp_part, float* scratch, int B, int heads, int ch, int c, bool softmax, hipStream_t s);
int launch_mdta_dtemp_reduce(const float* part, float* dtemp, int B, int heads, hipStream_t s);
// GDFN weight packs with the hidden width padded to hp (modes of gdfn_pack_kernel / gdfn_unpack_kernel)
int launch_gdfn_pack(const float* in, float* out, int c, int h, int hp, int mode, hipStream_t s);
int launch_gdfn_unpack(const float* in, float* out, int c, int h, int hp, int mode, hipStream_t s);

// ---- metrics.hip --------------------------------------------------------------------------
// PSNR / SSIM sums of NCHW image pairs (dcpt_imgmetric).  One workgroup per METRIC_TH x METRIC_TW tile of SSIM-map positions of one
// (image, scored channel); each writes one partial into ssim_part / sse_part [B * C'][metric_num_tiles], a second kernel adds them.
#define METRIC_TH 16
#define METRIC_TW 32
int metric_num_tiles(int Hc, int Wc);
int launch_imgmetric(const float* img, const float* img2, void* sse_out, double* ssim_out, double* ssim_part, void* sse_part, int B, int C,
                     int H, int W, int crop, int luma, int range, int want_ssim, hipStream_t s);

// ---- metrics_ms.hip -----------------------------------------------------------------------
// MS-SSIM (dcpt_msssim): one launch over (tile, image, level) on metrics.hip's tile, level k after k box passes in LDS; part holds
// [B][levels][metric_num_tiles][2] sums of the SSIM and CS maps, out [B][levels][2].  MATLAB SSIM (dcpt_ssim_matlab): the window at every
// pixel under replicate padding; part [B * C'][ssim_matlab_num_tiles], out [B][C'].  Range (dcpt_imgrange): min / max of the scored values of
// one image; part [B][imgrange_num_chunks][2], out [B][2].  Each is a tile kernel plus a fixed-order reduce.
#define MSSSIM_MAX_LEVELS 8
#define METRIC_RANGE_CHUNK 4096
int ssim_matlab_num_tiles(int Hc, int Wc);
int64_t imgrange_num_chunks(int Cp, int Hc, int Wc);
int launch_msssim(const float* img, const float* img2, double* out, double* part, int B, int C, int H, int W, int crop, int luma, int range,
                  int levels, hipStream_t s);
int launch_ssim_matlab(const float* img, const float* img2, double* out, double* part, int B, int C, int H, int W, int crop, int luma, int range,
                       hipStream_t s);
int launch_imgrange(const float* img, double* out, double* part, int B, int C, int H, int W, int crop, int luma, int range, hipStream_t s);

// ---- ssim_loss.hip --------------------------------------------------------------------------
// SSIM as a loss (dcpt_ssim_loss_fwd / _bwd): the forward writes one partial per tile into part[B * C'][ssim_loss_num_tiles]; the backward
// keeps Pa, Pb, Pc of ssim_loss_chunk_images images at a time in planes (ssim_loss_plane_bytes per image).
extern "C" size_t dcpt_ssim_loss_plane_cap;   // bytes of planes held at a time (64 MiB; a data symbol for the tests, not in the ABI)
int ssim_loss_num_tiles(int Hc, int Wc);
size_t ssim_loss_plane_bytes(int Cp, int Hc, int Wc);
int ssim_loss_chunk_images(int B, int Cp, int Hc, int Wc);
int launch_ssim_loss_fwd(const float* pred, const float* target, double* ssim_sum, double* part, int B, int C, int H, int W, int crop, int luma,
                         double range, hipStream_t s);
int launch_ssim_loss_bwd(const float* pred, const float* target, const double* gscale, float* dpred, double* planes, int B, int C, int H, int W,
                         int crop, int luma, double range, hipStream_t s);

// ---- ldl.hip --------------------------------------------------------------------------------
// The LDL artifact-weight map (dcpt_ldl_weight_fwd / _bwd).  The workspace, all fp64: scal = m, s, sum(Gz), sum(Gz z); part = two rows of
// ldl_num_partials per-workgroup partials (one per tile of the tile kernel, one per LDL_CHUNK elements of the element-wise kernels);
// u, mu = the forward's planes, which the backward reads; gv, gvmu = the backward's planes.
#define LDL_CHUNK 4096
struct LdlWs {
    double *scal, *part, *u, *mu, *gv, *gvmu;
};
int64_t ldl_num_partials(int B, int C, int H, int W);
int launch_ldl_weight_fwd(const float* gt, const float* out, float* w, const LdlWs& ws, int B, int C, int H, int W, hipStream_t s);
int launch_ldl_weight_bwd(const float* gt, const float* out, const float* gw, float* dout, const LdlWs& ws, int B, int C, int H, int W,
                          hipStream_t s);

// ---- jpeg.hip -------------------------------------------------------------------------------
// The DiffJPEG round trip (dcpt_diffjpeg_fwd): x, y fp32 NCHW planes, quality [B] on the device; one launch, no workspace.
int launch_diffjpeg_fwd(const float* x, const float* quality, float* y, int B, int C, int H, int W, int flags, hipStream_t s);

// ---- niqe.hip -------------------------------------------------------------------------------
// MATLAB-bicubic resize (dcpt_imresize_fwd): t is the fp64 intermediate [P][Ho][W].  NIQE (dcpt_niqe_mscn_fwd, dcpt_niqe_block_stats_fwd):
// the fp64 MSCN plane [P][Hc][Wc] of the cropped region and the [P][nblk][5][6] sums per block.
int launch_imresize_fwd(const void* x, void* y, const int* first_h, const double* w_h, const int* first_w, const double* w_w, double* t, int P,
                        int H, int W, int Ho, int Wo, int Kh, int Kw, int64_t plane_stride, int64_t row_stride, int x_f64, int y_f64,
                        int quant, hipStream_t s);
int launch_niqe_mscn_fwd(const void* x, double* n, int P, int H, int W, int crop, int Hc, int Wc, int scale, hipStream_t s);
int launch_niqe_block_stats_fwd(const double* n, double* stats, int P, int H, int W, int block, hipStream_t s);

// ---- degrade.hip ----------------------------------------------------------------------------
// The demosaic (dcpt_demosaic_fwd: x [B][C][H][W] with C = 1 the CFA plane or C = 3 an RGB image mosaicked while loading, y [B][3][H][W]) and
// the line-mask inpainting degradation (dcpt_inpaint_lines_fwd: lines int32 [B][10][4], meta int32 [B][3]); one launch each, no workspace.
int launch_demosaic_fwd(const float* x, float* y, int B, int C, int H, int W, int flags, hipStream_t s);
int launch_inpaint_lines_fwd(const float* x, const int* lines, const int* meta, float* y, int B, int C, int H, int W, hipStream_t s);

// ---- noise.hip ------------------------------------------------------------------------------
// Gaussian noise from a Philox4x32-10 stream per image (dcpt_gauss_noise_fwd: sigma fp32 [B], key int64 [B], gray int32 [B] or null on the
// device; x may be null with DCPT_NOISE_ONLY; in place allowed); one launch, no workspace.
int launch_gauss_noise_fwd(const float* x, const float* sigma, const long long* key, const int* gray, float* y, int B, int C, int H, int W,
                           int flags, hipStream_t s);
// Poisson (shot) noise on the same stream (dcpt_poisson_noise_fwd: scale fp32 [B]; x is always read): the level-count pass and the sampler,
// two launches; ws holds vals int32 [B] at its head and one 256-bit mask per (image, chunk) behind it (poisson_noise_ws_bytes, shape-only).
size_t poisson_noise_ws_bytes(int B, int C, int H, int W);
int launch_poisson_noise_fwd(const float* x, const float* scale, const long long* key, const int* gray, float* y, void* ws, int B, int C, int H,
                             int W, int flags, hipStream_t s);

// ---- blur.hip -------------------------------------------------------------------------------
// The K x K correlation of every plane with its image's kernel under reflect padding (dcpt_filter2d_fwd: kern fp32 [B][K][K], or [1][K][K]
// with per_image == 0; K odd, 1..51, K / 2 < H, W); fp64 accumulation in the tap order of the header; one launch, no workspace.
int launch_filter2d_fwd(const float* x, const float* kern, float* y, int B, int C, int H, int W, int K, int per_image, hipStream_t s);

// ---- resize.hip -----------------------------------------------------------------------------
// F.interpolate's area / bilinear / bicubic resize of dense NCHW fp32 planes (dcpt_interp_fwd: mode 0 / 1 / 2, the ratios are source pixels
// per destination pixel); fp64 taps and sums in the header's order; one launch, no workspace.
int launch_interp_fwd(const float* x, float* y, int B, int C, int H, int W, int Ho, int Wo, int mode, double ratio_h, double ratio_w, int flags,
                      hipStream_t s);

// ---- knn.hip --------------------------------------------------------------------------------
// Squared Euclidean distances between the rows of two fp32 / bf16 matrices in fp64 (dcpt_pdist2_fwd): the k-range in `ksplit` >= 1 chunks,
// partial norms, partial 64 x 64 tiles on the fp64 MFMA and the finishing pass: four launches; ws holds the partial tiles [ksplit][Nq][Nt]
// and the partial norms [ksplit][Nq], [ksplit][Nt] behind them (pdist2_ws_bytes, shape-only).  pdist2_auto_ksplit: the count for ksplit 0.
constexpr int PDIST2_MAX_KSPLIT = 65535, PDIST2_MAX_ROWS = 65535;
int pdist2_auto_ksplit(int Nq, int Nt, int64_t D);
size_t pdist2_ws_bytes(int Nq, int Nt, int ksplit);
int launch_pdist2_fwd(const void* xq, const void* xt, double* d2, void* ws, int Nq, int Nt, int64_t D, int64_t ldq, int64_t ldt, int64_t ldd,
                      int ksplit, int bf16, hipStream_t s);
// The k nearest training columns of every query row and their majority label, S splits in one launch (dcpt_knn_vote_fwd); no workspace.
int launch_knn_vote_fwd(const double* d2, int64_t ldd, const int* q_idx, const int* t_idx, const int* labels, int S, int nq, int nt, int k, int* nbr,
                        double* nbr_d2, int* pred, hipStream_t s);

// ---- tsne.hip -------------------------------------------------------------------------------
// Exact t-SNE on an fp64 squared-distance matrix (dcpt_tsne_*_fwd): the perplexity search per row, the symmetric joint probabilities, and
// descent iterations of two plain launches each.  One workspace layout serves the joint pass (N row sums) and the descent (the second
// embedding buffer and three per-row partials): tsne_ws_bytes, shape-only.
constexpr int TSNE_MAX_ROWS = 65535;
size_t tsne_ws_bytes(int N);
int launch_tsne_affinity_fwd(const double* d2, int64_t ldd, double* pcond, int64_t ldp, double* beta, int* steps, int N, double perplexity,
                             hipStream_t s);
int launch_tsne_joint_fwd(const double* pcond, int64_t ldp, double* P, int64_t ldo, void* ws, int N, hipStream_t s);
int launch_tsne_steps_fwd(const double* P, int64_t ldp, double* Y, double* update, double* gains, double* stats, void* ws, int N, int n_steps,
                          double exaggeration, double momentum, double lr, double min_gain, hipStream_t s);
int launch_tsne_kl_fwd(const double* P, int64_t ldp, const double* Y, double* grad, double* stats, void* ws, int N, double exaggeration,
                       hipStream_t s);
