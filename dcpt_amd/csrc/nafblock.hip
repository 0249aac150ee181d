// NAFBlock forward / backward composition (reference basicsr/archs/nafnet_arch.py:165-186).
//
// Forward (NHWC, M = B*H*W pixels):
//   xn1 = LN1(inp), stats1                                   ln_fwd (kept for conv1's weight gradient)
//   t1  = conv1(xn1)                                         gemm_nt<A_PLAIN, E_BIAS>  (operands by LDS-DMA)
//   t2  = SG(dw3x3(t1)+b2), pool partial sums                dw_fwd
//   s   = Wsca * mean(t2) + bsca                             sca_fwd
//   y   = inp + (conv3(t2*s)+b3)*beta                        gemm_nt<A_SCALE, E_RESID>
//   xn2 = LN2(y), stats2                                     ln_fwd
//   v   = conv4(xn2)                                         gemm_nt<A_PLAIN, E_BIAS>
//   (v's GEMM epilogue also writes g = SG(v))                gemm_nt<A_PLAIN, E_BIASGATE>
//   out = y + (conv5(g)+b5)*gamma                            gemm_nt<A_PLAIN, E_RESID>
//
// Backward never materialises the conv3/conv5 outputs: with G[n][k] = sum_m dO[m][n]*A'[m][k]
// (the un-scaled weight gradient) one has  dW = gain[n]*G,  dgain[n] = sum_k W[n][k]*G[n][k] +
// b[n]*sum_m dO[m][n],  db = gain[n]*sum_m dO[m][n]   (gain = beta or gamma), which also stays exact
// for the reference's zero-initialised beta/gamma.
#include "gemm.h"
#include "kernels.h"
#include "ffn_f32.h"
#include "side.h"
#include "../../include/dcpt_hip.h"

namespace {

struct FwdWs {
    float* w2p;
    float* pool_part;
    int nblk_pool;
};

size_t fwd_ws_layout(int B, int H, int W, int C, void* base, size_t bytes, FwdWs* out) {
    WsAlloc a(base, bytes);
    DwGeom g{B, H, W, C};
    const int nblk = dw_ring_num_blocks_per_image(g, 4);
    float* w2p = a.get<float>((size_t)9 * 2 * C);
    float* pp = a.get<float>((size_t)B * nblk * C);
    if (out) {
        out->w2p = w2p;
        out->pool_part = pp;
        out->nblk_pool = nblk;
    }
    return a.off;
}

struct BwdWs {
    float *wT5, *wT4, *wT3, *wT1, *w2p;
    float *b2a, *b2b, *b2c; // [M][2C]
    float *bca, *bcb, *bcc; // [M][C]
    float* slab;
    float* colsum;
    size_t slab_elems, colsum_elems;
    float *lnpart, *lnpart2;
    float *ds_part, *ds, *dpool;
    float* wpart;
    int ln_nblk, nblk_b;
    float* ffn_part;    // LayerNorm2 column partials of the fused narrowest-level backward (ffn_f32.hip): [waves][2][C]
};

bool ln_in_epilogue(int C);
bool ffn_fused_f32(int C);
size_t bwd_ws_layout(int B, int H, int W, int C, void* base, size_t bytes, BwdWs* out) {
    WsAlloc a(base, bytes);
    const int64_t M = (int64_t)B * H * W;
    const int P = H * W;
    DwGeom g{B, H, W, C};
    BwdWs w;
    w.wT5 = a.get<float>((size_t)C * C);
    w.wT4 = a.get<float>((size_t)2 * C * C);
    w.wT3 = a.get<float>((size_t)C * C);
    w.wT1 = a.get<float>((size_t)2 * C * C);
    w.w2p = a.get<float>((size_t)18 * C);
    w.b2a = a.get<float>((size_t)M * 2 * C);
    w.b2b = a.get<float>((size_t)M * 2 * C);
    w.b2c = a.get<float>((size_t)M * 2 * C);
    w.bca = a.get<float>((size_t)M * C);
    w.bcb = a.get<float>((size_t)M * C);
    w.bcc = a.get<float>((size_t)M * C);
    // slabs: the largest of (N=2C,K=C) and (N=C,K=C) plans
    int sp1, sp2;
    int64_t r1, r2;
    gemm_tn_plan(M, 2 * C, C, &sp1, &r1);
    gemm_tn_plan(M, C, C, &sp2, &r2);
    size_t slab1 = (size_t)sp1 * 2 * C * C, slab2 = (size_t)sp2 * C * C;
    size_t cs1 = (size_t)sp1 * gemm_tn_tiles_k(2 * C, C) * 2 * C, cs2 = (size_t)sp2 * gemm_tn_tiles_k(C, C) * C;
    {   // the image-aligned plan of conv3's weight gradient may use more splits
        int sp3;
        int64_t r3;
        if (gemm_tn_plan_images(M, C, C, P, &sp3, &r3)) {
            const size_t s3 = (size_t)sp3 * C * C, c3 = (size_t)sp3 * gemm_tn_tiles_k(C, C) * C;
            if (s3 > slab2) slab2 = s3;
            if (c3 > cs2) cs2 = c3;
        }
    }
    w.slab_elems = slab1 > slab2 ? slab1 : slab2;
    w.colsum_elems = cs1 > cs2 ? cs1 : cs2;
    w.slab = a.get<float>(w.slab_elems);
    w.colsum = a.get<float>(w.colsum_elems);
    w.ln_nblk = ln_bwd_num_blocks(M, C);
    {
        // LayerNorm column partials: [ln_nblk][3][C] from ln_bwd, or [M / 128 tiles][2][C] from the E_LNBWD GEMM epilogue
        const size_t a1 = (size_t)w.ln_nblk * 3 * C, a2 = (size_t)cdiv64(M, 128) * 2 * C;   // E_LNBWD tiles
        w.lnpart = a.get<float>(a1 > a2 ? a1 : a2);
        w.lnpart2 = a.get<float>(a1 > a2 ? a1 : a2);
    }
    {
        const int fs = sca_ds_fused_slices(P), ns = sca_ds_num_blocks(P);
        w.ds_part = a.get<float>((size_t)B * (fs > ns ? fs : ns) * C);
    }
    w.ds = a.get<float>((size_t)B * C);
    w.dpool = a.get<float>((size_t)B * C);
    w.nblk_b = dw_ring_bwd_num_blocks_per_image(g);   // tap-gradient partials of the fused depthwise backward
    w.wpart = a.get<float>((size_t)B * w.nblk_b * 10 * 2 * C);
    w.ffn_part = ffn_fused_f32(C) ? a.get<float>((size_t)ffn_bwd_f32_waves(M) * 2 * C) : nullptr;
    if (out) *out = w;
    return a.off;
}

// Narrow levels (C <= 128: one GEMM tile spans all channels): LayerNorm backward runs inside the epilogue of the dgrad GEMM
// that produces its incoming gradient, so that gradient is never written and re-read (2 tensor passes and one launch per
// LayerNorm).  DCPT_LN_EPILOGUE=0 switches back to the separate kernel.
// Narrowest level (C = 64): LayerNorm1 -> conv1 and LayerNorm2 -> conv4 -> SimpleGate -> conv5 -> residual as one pass each (ffn_f32.hip).
// The normalised tensors and the gate are then never written: the two weight-gradient GEMMs that read them take them from their
// operand loaders (A_LN on the LayerNorm's input, A_SG on v).
bool ffn_fused_f32(int C) {
    static const int on = dcpt_tuning("DCPT_FFN_FUSED_F32", 1);
    return on && ffn_fwd_f32_ok(C);
}

bool ln_in_epilogue(int C) {
    static const int on = dcpt_tuning("DCPT_LN_EPILOGUE", 1);
    return on && C <= 128;
}

}  // namespace

extern "C" int dcpt_nafblock_fused_ffn(int C) { return ffn_fused_f32(C) ? 1 : 0; }
extern "C" size_t dcpt_nafblock_fwd_ws_bytes(int B, int H, int W, int C) { return fwd_ws_layout(B, H, W, C, nullptr, 0, nullptr); }
extern "C" size_t dcpt_nafblock_bwd_ws_bytes(int B, int H, int W, int C) { return bwd_ws_layout(B, H, W, C, nullptr, 0, nullptr); }

extern "C" int dcpt_nafblock_fwd(const dcpt_nafblock_params* p, const float* inp, float* out, const dcpt_nafblock_saved* sv,
                                 void* ws, size_t ws_bytes, int B, int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && inp && out && sv, "nafblock_fwd: null argument");
    DCPT_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "nafblock_fwd: bad shape B=%d H=%d W=%d C=%d (B <= 65535, C %% 4 == 0)", B, H, W, C);
    FwdWs w;
    const size_t need = fwd_ws_layout(B, H, W, C, ws, ws_bytes, &w);
    DCPT_CHECK_WS("nafblock_fwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    const int P = H * W;
    const float eps = 1e-6f;  // nafnet_arch.py:57

    DCPT_CHECK_ARG(ffn_fused_f32(C) || (sv->xn1 && sv->xn2 && sv->g && sv->v && sv->mu1 && sv->rstd1 && sv->mu2 && sv->rstd2),
                   "nafblock_fwd: saved.xn1 / xn2 / g / v / statistics missing (optional only where dcpt_nafblock_fused_ffn(C) is 1)");
    DCPT_CHECK_ARG((sv->mu1 == nullptr) == (sv->rstd1 == nullptr) && (sv->mu2 == nullptr) == (sv->rstd2 == nullptr), "nafblock_fwd: mu / rstd come in pairs");
    // the normalised activations are materialised once: conv1's forward GEMM and (in backward) its weight-gradient GEMM
    // then take them as plain operands, i.e. straight global -> LDS by DMA
    const bool ffn = ffn_fused_f32(C);
    GemmNT g{};
    if (ffn) {
        FfnFwdF f{};
        f.y = inp; f.lnw = p->norm1_w; f.lnb = p->norm1_b; f.W4 = p->conv1_w; f.b4 = p->conv1_b; f.v = sv->t1; f.mu = sv->mu1; f.rstd = sv->rstd1;
        f.M = M; f.eps = eps;
        DCPT_TRY(launch_ln_conv_f32(f, C, s));
    } else {
        DCPT_TRY(launch_ln_fwd(inp, p->norm1_w, p->norm1_b, sv->xn1, sv->mu1, sv->rstd1, M, C, eps, s));
        g.M = M;
        // t1 = conv1(LN1(inp))
        g.A = sv->xn1; g.lda = C; g.K = C; g.Bw = p->conv1_w; g.N = 2 * C; g.C = sv->t1; g.ldc = 2 * C; g.bias = p->conv1_b;
        DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_BIAS, s));
    }
    // t2 = SG(dw(t1)+b2) and pooling partials
    DwGeom dg{B, H, W, C};
    DCPT_TRY(launch_dw_pack_weights(p->conv2_w, w.w2p, 2 * C, s));
    DCPT_TRY(launch_dw_ring_fwd_f32(sv->t1, w.w2p, p->conv2_b, sv->t2, w.pool_part, dg, s));
    DCPT_TRY(launch_sca_fwd(w.pool_part, w.nblk_pool, p->sca_w, p->sca_b, sv->pooled, sv->s, B, C, P, s));
    // y = inp + (conv3(t2*s)+b3)*beta
    g = GemmNT{};
    g.M = M; g.A = sv->t2; g.lda = C; g.K = C; g.Bw = p->conv3_w; g.N = C; g.C = sv->y; g.ldc = C;
    g.simg = sv->s; g.P = P; g.bias = p->conv3_b; g.res = inp; g.cscale = p->beta;
    if (ffn) {   // narrowest level: everything behind y is one kernel
        DCPT_TRY(launch_gemm_nt(g, A_SCALE, E_RESID, s));
        FfnFwdF f{};
        f.y = sv->y; f.lnw = p->norm2_w; f.lnb = p->norm2_b; f.W4 = p->conv4_w; f.b4 = p->conv4_b; f.W5 = p->conv5_w; f.b5 = p->conv5_b;
        f.gamma = p->gamma; f.out = out; f.v = sv->v; f.mu = sv->mu2; f.rstd = sv->rstd2; f.M = M; f.eps = eps;
        return launch_ffn_fwd_f32(f, C, s);
    }
    if (ln_in_epilogue(C)) {   // narrow levels: LN2(y) (statistics and normalised tensor) comes out of the same epilogue
        g.lnw = p->norm2_w; g.lnb = p->norm2_b; g.ln_out = sv->xn2; g.ln_mu = sv->mu2; g.ln_rstd = sv->rstd2; g.ln_eps = eps;
        DCPT_TRY(launch_gemm_nt(g, A_SCALE, E_RESIDLN, s));
    } else {
        DCPT_TRY(launch_gemm_nt(g, A_SCALE, E_RESID, s));
        DCPT_TRY(launch_ln_fwd(sv->y, p->norm2_w, p->norm2_b, sv->xn2, sv->mu2, sv->rstd2, M, C, eps, s));
    }
    // v = conv4(LN2(y))
    g = GemmNT{};
    g.M = M; g.A = sv->xn2; g.lda = C; g.K = C; g.Bw = p->conv4_w; g.N = 2 * C; g.C = sv->v; g.ldc = 2 * C; g.bias = p->conv4_b;
    g.gate = sv->g;   // the epilogue also emits SimpleGate(v), so conv5 (and its weight gradient) read a plain [M][C] operand
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_BIASGATE, s));
    // out = y + (conv5(SG(v))+b5)*gamma
    g = GemmNT{};
    g.M = M; g.A = sv->g; g.lda = C; g.K = C; g.Bw = p->conv5_w; g.N = C; g.C = out; g.ldc = C;
    g.bias = p->conv5_b; g.res = sv->y; g.cscale = p->gamma;
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_RESID, s));
    return DCPT_OK;
}

extern "C" int dcpt_nafblock_bwd(const dcpt_nafblock_params* p, const dcpt_nafblock_grads* gr, const float* inp,
                                 const dcpt_nafblock_saved* sv, const float* dout, float* dinp, void* ws, size_t ws_bytes,
                                 int B, int H, int W, int C, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && gr && inp && sv && dout && dinp, "nafblock_bwd: null argument");
    DCPT_CHECK_ARG(sv->v && sv->mu1 && sv->rstd1 && sv->mu2 && sv->rstd2 && (ffn_fused_f32(C) || (sv->xn1 && sv->xn2 && sv->g)),
                   "nafblock_bwd: saved tensors missing");
    DCPT_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "nafblock_bwd: bad shape B=%d H=%d W=%d C=%d (B <= 65535, C %% 4 == 0)", B, H, W, C);
    BwdWs w;
    const size_t need = bwd_ws_layout(B, H, W, C, ws, ws_bytes, &w);
    DCPT_CHECK_WS("nafblock_bwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    const int P = H * W;
    const int C2 = 2 * C;
    DwGeom dg{B, H, W, C};

    // transposed (and gain-scaled) weights for the dgrad GEMMs
    // (one launch; the depthwise [2C][9] -> [9][2C] packing is a transpose as well)
    WpackJobs jobs{};
    jobs.n = 5;
    jobs.in[0] = p->conv5_w; jobs.out[0] = w.wT5; jobs.rs[0] = p->gamma; jobs.N[0] = C;  jobs.K[0] = C;
    jobs.in[1] = p->conv4_w; jobs.out[1] = w.wT4; jobs.rs[1] = nullptr;  jobs.N[1] = C2; jobs.K[1] = C;
    jobs.in[2] = p->conv3_w; jobs.out[2] = w.wT3; jobs.rs[2] = p->beta;  jobs.N[2] = C;  jobs.K[2] = C;
    jobs.in[3] = p->conv1_w; jobs.out[3] = w.wT1; jobs.rs[3] = nullptr;  jobs.N[3] = C2; jobs.K[3] = C;
    jobs.in[4] = p->conv2_w; jobs.out[4] = w.w2p; jobs.rs[4] = nullptr;  jobs.N[4] = C2; jobs.K[4] = 9;
    DCPT_TRY(launch_wpack_multi(jobs, s));

    float* dv = w.b2a;
    float* gln = w.bca;
    float* dy = w.bcb;
    float* dts = w.bcc;
    float* da = w.b2c;
    float* dt1 = w.b2b;
    Side* sd = side_for(s);
    hipStream_t sw = side_stream(sd, s);   // stream of the weight-gradient GEMMs
    DCPT_TRY(side_fork(sd, 0, s));      // dout / saved activations / packed weights are ready

    const bool lne = ln_in_epilogue(C);
    GemmNT g{};
    GemmTN tp{};
    const bool ffn = ffn_fused_f32(C);   // narrowest level: B1 + B3 + B5 as one pass (ffn_f32.hip); the forward kept neither LN outputs nor the gate
    if (ffn) {
        FfnBwdF f{};
        f.dout = dout; f.v = sv->v; f.y = sv->y; f.wT5 = w.wT5; f.wT4 = w.wT4; f.lnw = p->norm2_w; f.dv = dv; f.dy = dy; f.lnpart = w.ffn_part;
        f.M = M; f.eps = 1e-6f;
        DCPT_TRY(launch_ffn_bwd_f32(f, C, s));
    } else {
        // B1: dv = SG'(dout*gamma * W5; v)
        g.M = M; g.A = dout; g.lda = C; g.K = C; g.Bw = w.wT5; g.N = C; g.C = dv; g.ldc = C2; g.aux = sv->v;
        DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_SGBWD, s));
    }
    // B2: conv5 / gamma gradients
    tp = GemmTN{};
    if (ffn) DCPT_TRY(launch_wgrad(tp, A_SG, dout, C, C, sv->v, C2, C, M, w.slab, w.colsum, gr->conv5_w, gr->conv5_b, WR_PLAIN, sw,
                                   WgradGain{p->gamma, p->conv5_w, p->conv5_b, gr->gamma}));
    else
    DCPT_TRY(launch_wgrad(tp, A_PLAIN, dout, C, C, sv->g, C, C, M, w.slab, w.colsum, gr->conv5_w, gr->conv5_b, WR_PLAIN, sw,
                          WgradGain{p->gamma, p->conv5_w, p->conv5_b, gr->gamma}));
    DCPT_TRY(side_fork(sd, 1, s));      // dv
    // B3: grad w.r.t. LN2 output
    g = GemmNT{};
    const int ln_tiles = (int)cdiv64(M, 128);
    g.M = M; g.A = dv; g.lda = C2; g.K = C2; g.Bw = w.wT4; g.N = C; g.C = gln; g.ldc = C;
    if (ffn) {
        // (done above)
    } else if (lne) {   // B3 + B5 in one launch: dy = dout + LN2-backward(dv * W4^T)
        g.C = dy; g.res = sv->y; g.ldres = C; g.aux = dout; g.mu = sv->mu2; g.rstd = sv->rstd2; g.lnw = p->norm2_w; g.colpart = w.lnpart;
        DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_LNBWD, s));
    } else {
        DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_PLAIN, s));
    }
    // B4: conv4 gradients (Y = LN2(y), kept by the forward pass)
    tp = GemmTN{};
    if (ffn) {
        tp.mu = sv->mu2; tp.rstd = sv->rstd2; tp.lnw = p->norm2_w; tp.lnb = p->norm2_b;
        DCPT_TRY(launch_wgrad(tp, A_LN, dv, C2, C2, sv->y, C, C, M, w.slab, w.colsum, gr->conv4_w, gr->conv4_b, WR_PLAIN, sw));
    } else
    DCPT_TRY(launch_wgrad(tp, A_PLAIN, dv, C2, C2, sv->xn2, C, C, M, w.slab, w.colsum, gr->conv4_w, gr->conv4_b, WR_PLAIN, sw));
    // B5: dy = dout + LN2-backward
    if (!ffn && !lne) DCPT_TRY(launch_ln_bwd(gln, sv->y, sv->mu2, sv->rstd2, p->norm2_w, dout, dy, w.lnpart, w.ln_nblk, M, C, s));
    DCPT_TRY(side_fork(sd, 2, s));      // dy, LN2 partial sums
    if (ffn) DCPT_TRY(launch_colpart_reduce(w.ffn_part, ffn_bwd_f32_waves(M), 2, C, gr->norm2_w, gr->norm2_b, nullptr, sw));
    else if (lne) DCPT_TRY(launch_colpart_reduce(w.lnpart, ln_tiles, 2, C, gr->norm2_w, gr->norm2_b, nullptr, sw));
    else DCPT_TRY(launch_colpart_reduce(w.lnpart, w.ln_nblk, 3, C, gr->norm2_w, gr->norm2_b, nullptr, sw));
    // B6: dts = d(t2*s)
    // when an image is a whole number of 128-pixel GEMM tiles, SCA's ds[b][k] = sum_p dts * t2 comes out of this GEMM's epilogue
    // as per-tile column sums (one bandwidth pass and one launch less)
    const bool ds_fused = sca_ds_fused_slices(P) > 0;
    const int ds_slices = ds_fused ? sca_ds_fused_slices(P) : sca_ds_num_blocks(P);
    g = GemmNT{};
    g.M = M; g.A = dy; g.lda = C; g.K = C; g.Bw = w.wT3; g.N = C; g.C = dts; g.ldc = C;
    if (ds_fused) {
        g.res = sv->t2; g.ldres = C; g.colpart = w.ds_part;
        DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_DOTCOL, s));
    } else {
        DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_PLAIN, s));
    }
    // B7: conv3 / beta gradients (Y = t2*s)
    {
        // G = sum_m dy[m][n] * t2[m][k] * s[img(m)][k]: when every pixel chunk lies inside one image the scale leaves the
        // GEMM (both operands plain, by LDS-DMA) and weights the per-chunk slabs in the reducer instead
        GemmTN t{};
        t.X = dy; t.ldx = C; t.N = C; t.Y = sv->t2; t.ldy = C; t.K = C; t.M = M; t.slab = w.slab; t.colsum = w.colsum;
        if (gemm_tn_plan_images(M, C, C, P, &t.splits, &t.rows_per_split) &&
            (size_t)t.splits * C * C <= w.slab_elems && (size_t)t.splits * gemm_tn_tiles_k(C, C) * C <= w.colsum_elems) {
            DCPT_TRY(launch_gemm_tn(t, A_PLAIN, A_PLAIN, sw));
            DCPT_TRY(launch_wgrad_reduce_scaled(w.slab, w.colsum, t.splits, t.splits * gemm_tn_tiles_k(C, C), C, C, p->beta, p->conv3_w,
                                                p->conv3_b, gr->conv3_w, gr->beta, gr->conv3_b, WR_PLAIN, sv->s,
                                                (int)(P / t.rows_per_split), sw));
        } else {
            tp = GemmTN{};
            tp.simg = sv->s; tp.P = P;
            DCPT_TRY(launch_wgrad(tp, A_SCALE, dy, C, C, sv->t2, C, C, M, w.slab, w.colsum, gr->conv3_w, gr->conv3_b, WR_PLAIN, sw,
                                  WgradGain{p->beta, p->conv3_w, p->conv3_b, gr->beta}));
        }
    }
    // B8: SCA backward
    if (!ds_fused) DCPT_TRY(launch_sca_ds_part(dts, sv->t2, w.ds_part, B, C, P, s));
    DCPT_TRY(launch_sca_dpool(w.ds_part, ds_slices, p->sca_w, w.dpool, B, C, P, s));
    // B9/B10: SimpleGate + depthwise conv backward
    (void)da;   // the fused kernel keeps da on chip
    DCPT_TRY(launch_dw_ring_bwd_fused_f32(dts, sv->t1, w.w2p, p->conv2_b, sv->s, w.dpool, dt1, w.wpart, dg, s));   // dwring.hip: every quantity computed once, rows by LDS-DMA
    DCPT_TRY(side_fork(sd, 3, s));      // dt1, depthwise and SCA partial sums
    DCPT_TRY(launch_sca_wgrad(w.ds_part, ds_slices, w.ds, sv->pooled, gr->sca_w, gr->sca_b, B, C, sw));
    DCPT_TRY(launch_dw_wgrad_reduce(w.wpart, B * w.nblk_b, C2, gr->conv2_w, gr->conv2_b, sw));
    // B11: grad w.r.t. LN1 output
    g = GemmNT{};
    g.M = M; g.A = dt1; g.lda = C2; g.K = C2; g.Bw = w.wT1; g.N = C; g.C = gln; g.ldc = C;
    if (lne) {   // B11 + B13 in one launch: dinp = dy + LN1-backward(dt1 * W1^T)
        g.C = dinp; g.res = inp; g.ldres = C; g.aux = dy; g.mu = sv->mu1; g.rstd = sv->rstd1; g.lnw = p->norm1_w; g.colpart = w.lnpart2;
        DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_LNBWD, s));
    } else {
        DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_PLAIN, s));
    }
    // B12: conv1 gradients (Y = LN1(inp), kept by the forward pass)
    tp = GemmTN{};
    if (ffn) {
        tp.mu = sv->mu1; tp.rstd = sv->rstd1; tp.lnw = p->norm1_w; tp.lnb = p->norm1_b;
        DCPT_TRY(launch_wgrad(tp, A_LN, dt1, C2, C2, inp, C, C, M, w.slab, w.colsum, gr->conv1_w, gr->conv1_b, WR_PLAIN, sw));
    } else
    DCPT_TRY(launch_wgrad(tp, A_PLAIN, dt1, C2, C2, sv->xn1, C, C, M, w.slab, w.colsum, gr->conv1_w, gr->conv1_b, WR_PLAIN, sw));
    // B13: dinp = dy + LN1-backward
    if (!lne) DCPT_TRY(launch_ln_bwd(gln, inp, sv->mu1, sv->rstd1, p->norm1_w, dy, dinp, w.lnpart2, w.ln_nblk, M, C, s));
    DCPT_TRY(side_fork(sd, 5, s));      // LN1 partial sums
    if (lne) DCPT_TRY(launch_colpart_reduce(w.lnpart2, ln_tiles, 2, C, gr->norm1_w, gr->norm1_b, nullptr, sw));
    else DCPT_TRY(launch_colpart_reduce(w.lnpart2, w.ln_nblk, 3, C, gr->norm1_w, gr->norm1_b, nullptr, sw));
    DCPT_TRY(side_join(sd, s));      // the caller's stream continues only after every weight gradient is written
    return DCPT_OK;
}

// ---------------------------------------------------------------------------------------------
// TLSC variant (reference nafnet_arch.py:277-288 NAFNet(Local_Base) + arch_util.py:313-455): inference-only forward in
// which SCA's global mean is a local k1 x k2 box mean, so the channel-attention scale is a per-pixel map:
//   smap = Wsca * boxmean(t2) + bsca (1x1 conv = MFMA GEMM),  x = t2 * smap  (GEMM epilogue E_MUL)
namespace {
struct LocalWs {
    float *w2p, *pool_part, *t1, *t2, *rowsum, *mmap, *t2s, *y, *v, *stats, *xn;
    int nblk_pool;
};
size_t local_layout(int B, int H, int W, int C, int k2, void* base, size_t bytes, LocalWs* out) {
    WsAlloc a(base, bytes);
    const int64_t M = (int64_t)B * H * W;
    DwGeom g{B, H, W, C};
    LocalWs w{};
    w.nblk_pool = dw_num_blocks_per_image(g);
    w.w2p = a.get<float>((size_t)18 * C);
    w.pool_part = a.get<float>((size_t)B * w.nblk_pool * C);
    w.t1 = a.get<float>((size_t)M * 2 * C);
    w.t2 = a.get<float>((size_t)M * C);
    w.rowsum = a.get<float>((size_t)B * H * (W - k2 + 1) * C);
    w.mmap = a.get<float>((size_t)M * C);
    w.t2s = a.get<float>((size_t)M * C);
    w.y = a.get<float>((size_t)M * C);
    w.v = w.t1;  // t1 is dead once t2 exists
    w.stats = a.get<float>((size_t)2 * M);
    w.xn = w.mmap;  // LN1(inp) is dead before the box mean is written, LN2(y) is formed after it was consumed
    if (out) *out = w;
    return a.off;
}
}  // namespace

extern "C" size_t dcpt_nafblock_local_ws_bytes(int B, int H, int W, int C, int k1, int k2) {
    (void)k1;
    return local_layout(B, H, W, C, k2 < W ? k2 : W, nullptr, 0, nullptr);
}

extern "C" int dcpt_nafblock_local_fwd(const dcpt_nafblock_params* p, const float* inp, float* out, void* ws, size_t ws_bytes, int B,
                                       int H, int W, int C, int k1, int k2, dcpt_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DCPT_CHECK_ARG(p && inp && out, "nafblock_local_fwd: null argument");
    DCPT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && k1 >= 1 && k2 >= 1, "nafblock_local_fwd: bad shape");
    if (k1 > H) k1 = H;   // arch_util.py:381 k = min(size, kernel)
    if (k2 > W) k2 = W;
    LocalWs w;
    const size_t need = local_layout(B, H, W, C, k2, ws, ws_bytes, &w);
    DCPT_CHECK_WS("nafblock_local_fwd", ws, ws_bytes, need);
    const int64_t M = (int64_t)B * H * W;
    float* mu = w.stats;
    float* rstd = w.stats + M;
    DCPT_TRY(launch_ln_fwd(inp, p->norm1_w, p->norm1_b, w.xn, mu, rstd, M, C, 1e-6f, s));
    GemmNT g{};
    g.M = M; g.A = w.xn; g.lda = C; g.K = C; g.Bw = p->conv1_w; g.N = 2 * C; g.C = w.t1; g.ldc = 2 * C; g.bias = p->conv1_b;
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_BIAS, s));
    DwGeom dg{B, H, W, C};
    DCPT_TRY(launch_dw_pack_weights(p->conv2_w, w.w2p, 2 * C, s));
    DCPT_TRY(launch_dw_fwd(w.t1, w.w2p, p->conv2_b, w.t2, w.pool_part, dg, s));
    DCPT_TRY(launch_box_mean(w.t2, w.rowsum, w.mmap, B, H, W, C, k1, k2, s));
    g = GemmNT{};
    g.M = M; g.A = w.mmap; g.lda = C; g.K = C; g.Bw = p->sca_w; g.N = C; g.C = w.t2s; g.ldc = C; g.bias = p->sca_b; g.res = w.t2;
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_MUL, s));
    g = GemmNT{};
    g.M = M; g.A = w.t2s; g.lda = C; g.K = C; g.Bw = p->conv3_w; g.N = C; g.C = w.y; g.ldc = C;
    g.bias = p->conv3_b; g.res = inp; g.cscale = p->beta;
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_RESID, s));
    DCPT_TRY(launch_ln_fwd(w.y, p->norm2_w, p->norm2_b, w.xn, mu, rstd, M, C, 1e-6f, s));
    g = GemmNT{};
    g.M = M; g.A = w.xn; g.lda = C; g.K = C; g.Bw = p->conv4_w; g.N = 2 * C; g.C = w.v; g.ldc = 2 * C; g.bias = p->conv4_b;
    g.gate = w.t2s;   // t2*smap is dead once y exists
    DCPT_TRY(launch_gemm_nt(g, A_PLAIN, E_BIASGATE, s));
    g = GemmNT{};
    g.M = M; g.A = w.t2s; g.lda = C; g.K = C; g.Bw = p->conv5_w; g.N = C; g.C = out; g.ldc = C;
    g.bias = p->conv5_b; g.res = w.y; g.cscale = p->gamma;
    return launch_gemm_nt(g, A_PLAIN, E_RESID, s);
}
