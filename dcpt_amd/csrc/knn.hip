// The kNN degradation probe (include/dcpt_hip.h dcpt_pdist2_fwd, dcpt_knn_vote_fwd): squared Euclidean distances between the rows of two
// matrices in fp64 on the fp64 matrix cores, and the k-nearest-neighbour majority vote over them.
//
// Distances.  N is a few hundred and D is 10^5 .. 10^6, so the output has a handful of 64 x 64 tiles and the k-range is cut into
// `ksplit` chunks of L = 4 ceil(ceil(D / 4) / ksplit) elements (the last ones ragged or empty); chunk c covers k in [c L, min(D, (c + 1) L)).
// Three kernels, no atomics, every store a plain store:
//   pdist2_norm_kernel   grid (rows, ksplit): the partial squared norm of one row over one chunk.  Lane t of the 256 sums the elements
//                        c L + t, + 256, ... in that order; the 256 sums are added by a fixed binary tree in LDS.
//   pdist2_gemm_kernel   grid (tiles, ksplit): the partial 64 x 64 tile of G = Q T^t over one chunk.  Per step of KT = 32 columns a
//                        workgroup loads 64 rows of each operand (8 consecutive elements per lane), converts every element ONCE to fp64
//                        and stores it to LDS; each of the four waves owns a 32 x 32 quarter as 2 x 2 v_mfma_f64_16x16x4_f64 tiles, so an
//                        operand fragment read from LDS (one f64 per lane) feeds two MFMAs.  The next step's global loads are in flight
//                        while the current one multiplies.  Rows past Nq / Nt and columns past the chunk are zeros: x + 0 is x, so they
//                        change no bit of a real element.  The tile goes to ws[c][i][j].
//   pdist2_finish_kernel one lane per (i, j): G, n_i, m_j as the sums of their partials in chunk order, then max(0, (n + m) - 2 G).
// An accumulator element sees its row's and its column's products in the order of k and nothing else, whatever its place in the tile, the
// tile's place in the matrix or the leading dimensions: that is the contract of the header (permuted rows give permuted bits).
// The f64 MFMA's C/D map is col = lane & 15, row = (lane >> 4) + 4 reg -- NOT the f32 16x16x4 map ((lane >> 4) * 4 + reg); A and B are one
// f64 per lane, A[lane & 15][k = lane >> 4] and B[k = lane >> 4][lane & 15].
//
// Vote.  One wave per (query, split).  The neighbours are ordered by (distance, position in t_idx), a strict total order, so the next
// neighbour is the smallest pair above the previous one: k rounds of a wave-wide lexicographic argmin, the taken ones masked by that
// comparison alone.  A distance becomes an unsigned key that orders as the numbers do (-0 as +0, every NaN above +inf).  Lane r keeps the
// label of neighbour r; the vote counts equal labels across lanes and takes (largest count, smallest label).
#include <stdint.h>

#include "kernels.h"
#include "prof.h"

namespace {
typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;            // lanes of a workgroup (four waves)
constexpr int TM = 64;             // the output tile is TM x TM
constexpr int KT = 32;             // columns of one LDS step
constexpr int LDS_LD = KT + 4;     // doubles per LDS row: 72 dwords, so a fragment read (16 rows x 4 columns of f64) spreads over all banks
constexpr int PROF_PDIST_NORM = PROF_OTHER + 10, PROF_PDIST_GEMM = PROF_OTHER + 11, PROF_PDIST_FINISH = PROF_OTHER + 12,
              PROF_KNN_VOTE = PROF_OTHER + 13;

struct PdistGeom {
    int Nq, Nt, ksplit, bf16;
    int64_t D, ldq, ldt, ldd, L;   // L: elements per chunk, a multiple of 4
    int vecq, vect;                // the operand's rows allow 16-byte (fp32) / 8-byte (bf16) loads of four elements at k % 4 == 0
};

template <bool BF>
__device__ __forceinline__ double elem(const void* p, int64_t i) {
    if constexpr (BF) return (double)__uint_as_float((uint32_t)((const uint16_t*)p)[i] << 16);
    else return (double)((const float*)p)[i];
}

// eight consecutive elements of a row from column k (below kend), as fp64; zeros past kend or for a row past the matrix
template <bool BF>
__device__ __forceinline__ void load8(const void* base, int64_t row_off, bool row_ok, int64_t k, int64_t kend, bool vec, double (&v)[8]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t kk = k + 4 * h;
        if (row_ok && vec && kk + 4 <= kend) {
            if constexpr (BF) {
                const uint2 w = *reinterpret_cast<const uint2*>((const uint16_t*)base + row_off + kk);
                v[4 * h + 0] = (double)__uint_as_float(w.x << 16);
                v[4 * h + 1] = (double)__uint_as_float(w.x & 0xffff0000u);
                v[4 * h + 2] = (double)__uint_as_float(w.y << 16);
                v[4 * h + 3] = (double)__uint_as_float(w.y & 0xffff0000u);
            } else {
                const float4 w = *reinterpret_cast<const float4*>((const float*)base + row_off + kk);
                v[4 * h + 0] = (double)w.x; v[4 * h + 1] = (double)w.y; v[4 * h + 2] = (double)w.z; v[4 * h + 3] = (double)w.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * h + j] = (row_ok && kk + j < kend) ? elem<BF>(base, row_off + kk + j) : 0.0;
        }
    }
}

template <bool BF>
__global__ __launch_bounds__(NT) void pdist2_gemm_kernel(const void* __restrict__ xq, const void* __restrict__ xt, double* __restrict__ part,
                                                         PdistGeom g) {
    __shared__ double sq[TM * LDS_LD];
    __shared__ double st[TM * LDS_LD];
    const int tiles_t = (g.Nt + TM - 1) / TM;
    const int ti = (int)blockIdx.x / tiles_t, tj = (int)blockIdx.x - ti * tiles_t;
    const int c = (int)blockIdx.y;
    const int64_t k0 = (int64_t)c * g.L;
    const int64_t kend = k0 + g.L < g.D ? k0 + g.L : g.D;   // (k0 may lie past D: an empty chunk stores zeros)

    // loads: lane t takes row t / 4 of the tile and the columns 8 (t % 4) .. + 7 of the step, for both operands
    const int lr = (int)threadIdx.x >> 2, lk = ((int)threadIdx.x & 3) * 8;
    const int qi = ti * TM + lr, tjr = tj * TM + lr;
    const bool q_ok = qi < g.Nq, t_ok = tjr < g.Nt;
    const int64_t q_off = (int64_t)qi * g.ldq, t_off = (int64_t)tjr * g.ldt;

    // MFMA: wave w owns rows 32 (w / 2) .. + 31 and columns 32 (w % 2) .. + 31 of the tile
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int fr = lane & 15, fk = lane >> 4;
    doublex4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = doublex4{0.0, 0.0, 0.0, 0.0};

    double vq[8], vt[8];
    if (k0 < kend) {
        load8<BF>(xq, q_off, q_ok, k0 + lk, kend, g.vecq != 0, vq);
        load8<BF>(xt, t_off, t_ok, k0 + lk, kend, g.vect != 0, vt);
    }
    for (int64_t k = k0; k < kend; k += KT) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sq[lr * LDS_LD + lk + j] = vq[j];
            st[lr * LDS_LD + lk + j] = vt[j];
        }
        __syncthreads();
        if (k + KT < kend) {   // the next step's loads fly while this one multiplies
            load8<BF>(xq, q_off, q_ok, k + KT + lk, kend, g.vecq != 0, vq);
            load8<BF>(xt, t_off, t_ok, k + KT + lk, kend, g.vect != 0, vt);
        }
#pragma unroll
        for (int s = 0; s < KT / 4; ++s) {
            const double a0 = sq[(wr + fr) * LDS_LD + 4 * s + fk], a1 = sq[(wr + 16 + fr) * LDS_LD + 4 * s + fk];
            const double b0 = st[(wc + fr) * LDS_LD + 4 * s + fk], b1 = st[(wc + 16 + fr) * LDS_LD + 4 * s + fk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();   // (the LDS step is rewritten)
    }

    // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
    double* out = part + (int64_t)c * g.Nq * g.Nt;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * TM + wr + 16 * a + (lane >> 4) + 4 * r, j = tj * TM + wc + 16 * b + (lane & 15);
                if (i < g.Nq && j < g.Nt) out[(int64_t)i * g.Nt + j] = acc[a][b][r];
            }
}

// npart[c][row]: the squared norm of a row over chunk c
template <bool BF>
__global__ __launch_bounds__(NT) void pdist2_norm_kernel(const void* __restrict__ x, double* __restrict__ npart, int N, int64_t ld, int64_t D,
                                                         int64_t L) {
    __shared__ double red[NT];
    const int row = (int)blockIdx.x, c = (int)blockIdx.y;
    const int64_t k0 = (int64_t)c * L;
    const int64_t kend = k0 + L < D ? k0 + L : D;
    const int64_t off = (int64_t)row * ld;
    double s = 0.0;
    for (int64_t k = k0 + threadIdx.x; k < kend; k += NT) {
        const double v = elem<BF>(x, off + k);
        s = fma(v, v, s);   // (the square of an fp32 value is exact in fp64: the same bits as a product and a sum)
    }
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = NT / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) npart[(int64_t)c * N + row] = red[0];
}

__global__ __launch_bounds__(NT) void pdist2_finish_kernel(const double* __restrict__ part, const double* __restrict__ nq, const double* __restrict__ nt,
                                                           double* __restrict__ d2, PdistGeom g) {
    const int i = (int)blockIdx.y;
    const int j = (int)blockIdx.x * NT + (int)threadIdx.x;
    if (j >= g.Nt) return;
    double G = 0.0, n = 0.0, m = 0.0;
    for (int c = 0; c < g.ksplit; ++c) {   // chunk order
        G = G + part[((int64_t)c * g.Nq + i) * g.Nt + j];
        n = n + nq[(int64_t)c * g.Nq + i];
        m = m + nt[(int64_t)c * g.Nt + j];
    }
    const double v = (n + m) - 2.0 * G;   // (2 G is exact)
    d2[(int64_t)i * g.ldd + j] = v < 0.0 ? 0.0 : v;   // (a NaN stays a NaN)
}

// ---- vote ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t order_key(double d) {
    if (d != d) return ~(uint64_t)0;          // every NaN ranks after every number (+inf is 0xfff0...)
    if (d == 0.0) return (uint64_t)1 << 63;   // -0 as +0
    const uint64_t b = (uint64_t)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | ((uint64_t)1 << 63));
}

__device__ __forceinline__ bool pair_less(uint64_t ka, int pa, uint64_t kb, int pb) { return ka < kb || (ka == kb && pa < pb); }

constexpr int VOTE_WAVES = 4;   // waves (queries) of a workgroup

__global__ __launch_bounds__(64 * VOTE_WAVES) void knn_vote_kernel(const double* __restrict__ d2, int64_t ldd, const int* __restrict__ q_idx,
                                                                   const int* __restrict__ t_idx, const int* __restrict__ labels, int S, int nq, int nt,
                                                                   int k, int* __restrict__ nbr, double* __restrict__ nbr_d2, int* __restrict__ pred) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * VOTE_WAVES + ((int)threadIdx.x >> 6);   // (query, split), the query fastest
    if (item >= (int64_t)S * nq) return;   // (a whole wave leaves: no lane of it takes part in a shuffle)
    const int s = (int)(item / nq);
    const int* ti = t_idx + (int64_t)s * nt;
    const double* row = d2 + (int64_t)q_idx[item] * ldd;
    constexpr int NONE = 0x7fffffff;
    uint64_t last_key = 0;
    int last_pos = -1;   // (no key is 0 -- the smallest, -inf, is 0x000f...ffff -- so every candidate lies above the start)
    int my_label = 0;
    for (int r = 0; r < k; ++r) {
        uint64_t bk = ~(uint64_t)0;
        int bp = NONE;
        for (int p = lane; p < nt; p += 64) {
            const uint64_t key = order_key(row[ti[p]]);
            if (pair_less(last_key, last_pos, key, p) && pair_less(key, p, bk, bp)) {
                bk = key;
                bp = p;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t ok = (uint64_t)__shfl_xor((unsigned long long)bk, d, 64);
            const int op = __shfl_xor(bp, d, 64);
            if (pair_less(ok, op, bk, bp)) {
                bk = ok;
                bp = op;
            }
        }
        // k <= nt: a candidate above the previous neighbour always exists, so bp is a position (the clamp only keeps a broken
        // invariant from becoming an address)
        if (bp >= nt) bp = nt - 1;
        last_key = bk;
        last_pos = bp;
        const int col = ti[bp];
        if (lane == r) my_label = labels[col];
        if (lane == 0) {
            nbr[item * k + r] = bp;
            nbr_d2[item * k + r] = row[col];
        }
    }
    // the vote: lane r < k holds the label of neighbour r
    int count = 0;
    for (int r = 0; r < k; ++r) count += __shfl(my_label, r, 64) == my_label ? 1 : 0;
    if (lane >= k) count = 0;
    int best_count = count, best_label = my_label;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int oc = __shfl_xor(best_count, d, 64), ol = __shfl_xor(best_label, d, 64);
        if (oc > best_count || (oc == best_count && oc > 0 && ol < best_label)) {
            best_count = oc;
            best_label = ol;
        }
    }
    if (lane == 0) pred[item] = best_label;
}

size_t pdist2_part_bytes(int Nq, int Nt, int ksplit) { return align_up((size_t)ksplit * Nq * Nt * sizeof(double), 256); }
size_t pdist2_norm_bytes(int N, int ksplit) { return align_up((size_t)ksplit * N * sizeof(double), 256); }
}  // namespace

int pdist2_auto_ksplit(int Nq, int Nt, int64_t D) {
    // about four workgroups for each of the 256 compute units, and chunks of at least 512 columns
    const int64_t tiles = cdiv64(Nq, TM) * cdiv64(Nt, TM);
    int64_t ks = cdiv64(1024, tiles);
    const int64_t cap = D / 512 > 1 ? D / 512 : 1;
    if (ks > cap) ks = cap;
    if (ks > PDIST2_MAX_KSPLIT) ks = PDIST2_MAX_KSPLIT;
    return (int)ks;
}

size_t pdist2_ws_bytes(int Nq, int Nt, int ksplit) {
    return pdist2_part_bytes(Nq, Nt, ksplit) + pdist2_norm_bytes(Nq, ksplit) + pdist2_norm_bytes(Nt, ksplit);
}

int launch_pdist2_fwd(const void* xq, const void* xt, double* d2, void* ws, int Nq, int Nt, int64_t D, int64_t ldq, int64_t ldt, int64_t ldd,
                      int ksplit, int bf16, hipStream_t s) {
    PdistGeom g{};
    g.Nq = Nq; g.Nt = Nt; g.ksplit = ksplit; g.bf16 = bf16;
    g.D = D; g.ldq = ldq; g.ldt = ldt; g.ldd = ldd;
    g.L = 4 * cdiv64(cdiv64(D, 4), ksplit);
    const uintptr_t amask = bf16 ? 7 : 15;   // four elements
    g.vecq = ((uintptr_t)xq & amask) == 0 && ldq % 4 == 0;
    g.vect = ((uintptr_t)xt & amask) == 0 && ldt % 4 == 0;
    double* part = (double*)ws;
    double* nq = (double*)((char*)ws + pdist2_part_bytes(Nq, Nt, ksplit));
    double* nt = (double*)((char*)nq + pdist2_norm_bytes(Nq, ksplit));
    const double esz = bf16 ? 2.0 : 4.0;
    {
        ProfScope prof(s, PROF_PDIST_NORM, (int64_t)(Nq + Nt) * D, 0, 0, 2.0 * (double)(Nq + Nt) * (double)D, esz * (double)(Nq + Nt) * (double)D);
        trace_tag("knn.pdist2_norm");
        if (bf16) {
            pdist2_norm_kernel<true><<<dim3((unsigned)Nq, (unsigned)ksplit), dim3(NT), 0, s>>>(xq, nq, Nq, ldq, D, g.L);
            pdist2_norm_kernel<true><<<dim3((unsigned)Nt, (unsigned)ksplit), dim3(NT), 0, s>>>(xt, nt, Nt, ldt, D, g.L);
        } else {
            pdist2_norm_kernel<false><<<dim3((unsigned)Nq, (unsigned)ksplit), dim3(NT), 0, s>>>(xq, nq, Nq, ldq, D, g.L);
            pdist2_norm_kernel<false><<<dim3((unsigned)Nt, (unsigned)ksplit), dim3(NT), 0, s>>>(xt, nt, Nt, ldt, D, g.L);
        }
        DCPT_CHECK_LAUNCH("pdist2_fwd (norms)");
    }
    {
        const unsigned tiles = (unsigned)(cdiv(Nq, TM) * cdiv(Nt, TM));   // at most 1024 x 1024
        ProfScope prof(s, PROF_PDIST_GEMM, (int64_t)Nq * Nt, 0, 0, 2.0 * (double)Nq * (double)Nt * (double)D,
                       esz * (double)tiles * 2.0 * TM * (double)D);
        trace_tag("knn.pdist2_gemm");
        if (bf16) pdist2_gemm_kernel<true><<<dim3(tiles, (unsigned)ksplit), dim3(NT), 0, s>>>(xq, xt, part, g);
        else pdist2_gemm_kernel<false><<<dim3(tiles, (unsigned)ksplit), dim3(NT), 0, s>>>(xq, xt, part, g);
        DCPT_CHECK_LAUNCH("pdist2_fwd (gemm)");
    }
    ProfScope prof(s, PROF_PDIST_FINISH, (int64_t)Nq * Nt, 0, 0, 0.0, 8.0 * (double)Nq * (double)Nt * (ksplit + 1));
    trace_tag("knn.pdist2_finish");
    pdist2_finish_kernel<<<dim3((unsigned)cdiv(Nt, NT), (unsigned)Nq), dim3(NT), 0, s>>>(part, nq, nt, d2, g);
    DCPT_CHECK_LAUNCH("pdist2_fwd (finish)");
    return DCPT_OK;
}

int launch_knn_vote_fwd(const double* d2, int64_t ldd, const int* q_idx, const int* t_idx, const int* labels, int S, int nq, int nt, int k, int* nbr,
                        double* nbr_d2, int* pred, hipStream_t s) {
    const int64_t items = (int64_t)S * nq;
    ProfScope prof(s, PROF_KNN_VOTE, items, 0, 0, 0.0, 8.0 * (double)items * (double)nt * k);
    trace_tag("knn.vote");
    knn_vote_kernel<<<dim3((unsigned)cdiv64(items, VOTE_WAVES)), dim3(64 * VOTE_WAVES), 0, s>>>(d2, ldd, q_idx, t_idx, labels, S, nq, nt, k, nbr,
                                                                                               nbr_d2, pred);
    DCPT_CHECK_LAUNCH("knn_vote_fwd");
    return DCPT_OK;
}
