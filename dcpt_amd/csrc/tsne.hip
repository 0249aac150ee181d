// Exact t-SNE of the probe's features (include/dcpt_hip.h dcpt_tsne_affinity_fwd, dcpt_tsne_joint_fwd, dcpt_tsne_steps_fwd, dcpt_tsne_kl_fwd):
// the rules of scikit-learn's method="exact" on an fp64 squared-distance matrix, all arithmetic fp64, plain launches, plain stores, no atomics.
// scikit-learn rounds the distances to float32 before the perplexity search; these kernels do not.
//
// Sums.  Two orders occur and nothing else:
//   block order  lane t of the 256 adds its terms j = t, t + 256, ... in ascending j; the 256 sums go through a fixed binary tree in LDS
//                (t += t + 128, then 64, ... 1): block_sum.h, shared with the metric and loss kernels.
//   wave order   lane t of the 64 adds its terms j = t, t + 64, ... in ascending j; the 64 sums go through the xor butterfly 32, 16, ... 1
//                (a + b and b + a are the same bits, so every lane ends with the same value).
// A row's result depends on that row's inputs and on N only: a row is owned by one workgroup (affinities, joint) or one wave (descent), and a
// value every row needs (S, Z) is re-added by every owner from per-row partials in the same order.
//
// Affinities.  affinity_kernel, one workgroup per row i: the binary search of the header on beta.  Per step a lane stores exp(-d2_ij beta) to its
// columns of pcond's row, the workgroup adds them (block order) to s, the SAME lane reads its columns back, divides by s, stores and adds
// d2_ij p_j (block order) to sd; every lane then takes the same decision from the same two numbers.  beta moves by doubling, halving and
// midpoints only: exact dyadic arithmetic, so beta and the step count equal any other exact evaluation unless a visited |e| lies at 1e-5.
// Joint.  joint_rowsum_kernel, one workgroup per row: r_i = sum_{j != i} (pcond_ij + pcond_ji), block order.  joint_kernel, one workgroup per
// row i: S = max(sum_k r_k, EPS) in block order over k, then the pairs (i, j), j > i: v = max((pcond_ij + pcond_ji) / S, EPS) goes to P_ij and
// P_ji.  A pair has one owner that reads both entries before it writes both, so P may be pcond, and P is symmetric bit for bit.
//
// Descent, two launches per iteration, one wave per row, four rows per workgroup; the (N, 2) embedding passes through LDS in tiles of 1024
// points (16 KiB) that the four waves share:
//   zrow_kernel   z_i = sum_{j != i} w_ij, w_ij = 1 / (1 + |y_i - y_j|^2), wave order.
//   grad_kernel   Z = sum_k z_k (wave order over k; every wave adds the N partials itself), then over j != i in wave order the two components of
//                 sum (P'_ij - Q_ij) w_ij (y_i - y_j) with Q_ij = max(w_ij / Z, EPS) -- w is computed again rather than stored: N^2 doubles per
//                 iteration would cost more than the division -- and, where asked, sum P'_ij log(max(P'_ij, EPS) / Q_ij).  Lane 0 applies the
//                 gain / momentum rule to its row and writes the new point to the OTHER embedding buffer, so no wave reads a row another writes.
//   stats_kernel  (last iteration only) one workgroup adds the per-row KL terms and squared gradient norms in block order.
// The second embedding buffer and the per-row partials live in the workspace; after an odd number of iterations the result is copied back.
#include <math.h>
#include <stdint.h>

#include "block_sum.h"
#include "kernels.h"
#include "prof.h"

namespace {
constexpr int NT = BLOCK_NT;   // lanes of a workgroup (four waves)
constexpr int ROWS = NT / 64;  // descent: rows (waves) of a workgroup
constexpr int YT = 1024;       // descent: points of one LDS tile, a multiple of 256
constexpr double EPS = 2.220446049250313080847263336181640625e-16;   // 2^-52
constexpr int PROF_TSNE_AFFINITY = PROF_OTHER + 14, PROF_TSNE_JOINT = PROF_OTHER + 15, PROF_TSNE_ZROW = PROF_OTHER + 16,
              PROF_TSNE_GRAD = PROF_OTHER + 17, PROF_TSNE_STATS = PROF_OTHER + 18;

// block order, second half: block_sum of block_sum.h.  wave order, second half:
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(NT) void affinity_kernel(const double* __restrict__ d2, int64_t ldd, double* __restrict__ pcond, int64_t ldp,
                                                      double* __restrict__ beta_out, int* __restrict__ steps_out, int N, double log_perp) {
    __shared__ double red[NT];
    const int i = (int)blockIdx.x, t = (int)threadIdx.x;
    const double* drow = d2 + (int64_t)i * ldd;
    double* prow = pcond + (int64_t)i * ldp;
    double beta = 1.0, lo = -INFINITY, hi = INFINITY;
    int l = 0;
    for (;; ++l) {   // (every lane holds the same beta, lo, hi and l: the decisions below are uniform)
        double part = 0.0;
        for (int j = t; j < N; j += NT)
            if (j != i) {
                const double p = exp(-drow[j] * beta);
                prow[j] = p;
                part = part + p;
            }
        double s = block_sum(part, red);
        if (s == 0.0) s = 1e-8;
        part = 0.0;
        for (int j = t; j < N; j += NT)
            if (j != i) {   // (a lane reads back what it stored itself)
                const double p = prow[j] / s;
                prow[j] = p;
                part = part + drow[j] * p;
            }
        const double sd = block_sum(part, red);
        const double e = log(s) + beta * sd - log_perp;
        if (fabs(e) <= 1e-5) break;
        if (e > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
        }
        if (l == 99) break;
    }
    if (t == 0) {
        prow[i] = 0.0;
        beta_out[i] = beta;
        steps_out[i] = l;
    }
}

__global__ __launch_bounds__(NT) void joint_rowsum_kernel(const double* __restrict__ pcond, int64_t ldp, double* __restrict__ rs, int N) {
    __shared__ double red[NT];
    const int i = (int)blockIdx.x;
    double part = 0.0;
    for (int j = (int)threadIdx.x; j < N; j += NT)
        if (j != i) part = part + (pcond[(int64_t)i * ldp + j] + pcond[(int64_t)j * ldp + i]);
    const double r = block_sum(part, red);
    if (threadIdx.x == 0) rs[i] = r;
}

// (no __restrict__: P may be pcond)
__global__ __launch_bounds__(NT) void joint_kernel(const double* pcond, int64_t ldp, double* P, int64_t ldo, const double* __restrict__ rs, int N) {
    __shared__ double red[NT];
    const int i = (int)blockIdx.x;
    double part = 0.0;
    for (int k = (int)threadIdx.x; k < N; k += NT) part = part + rs[k];
    double S = block_sum(part, red);
    if (!(S >= EPS)) S = EPS;
    for (int j = i + 1 + (int)threadIdx.x; j < N; j += NT) {
        double v = (pcond[(int64_t)i * ldp + j] + pcond[(int64_t)j * ldp + i]) / S;
        if (!(v >= EPS)) v = EPS;
        P[(int64_t)i * ldo + j] = v;
        P[(int64_t)j * ldo + i] = v;
    }
    if (threadIdx.x == 0) P[(int64_t)i * ldo + i] = 0.0;
}

// points t0 .. t0 + YT - 1 of the embedding into LDS (the whole workgroup)
__device__ __forceinline__ void stage_tile(const double* __restrict__ Y, double2* ys, int t0, int N) {
    __syncthreads();   // (the previous tile has been read)
#pragma unroll
    for (int k = 0; k < YT / NT; ++k) {
        const int p = (int)threadIdx.x + NT * k;
        if (t0 + p < N) ys[p] = reinterpret_cast<const double2*>(Y)[t0 + p];
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void zrow_kernel(const double* __restrict__ Y, double* __restrict__ zrow, int N) {
    __shared__ double2 ys[YT];
    const int lane = (int)threadIdx.x & 63;
    const int i = (int)blockIdx.x * ROWS + ((int)threadIdx.x >> 6);
    const bool row_ok = i < N;   // (a wave past the last row still stages tiles and meets the barriers)
    double2 yi = double2{0.0, 0.0};
    if (row_ok) yi = reinterpret_cast<const double2*>(Y)[i];
    double z = 0.0;
    for (int t0 = 0; t0 < N; t0 += YT) {
        stage_tile(Y, ys, t0, N);
        if (row_ok)
            for (int p = lane; p < YT && t0 + p < N; p += 64)
                if (t0 + p != i) {
                    const double dx = yi.x - ys[p].x, dy = yi.y - ys[p].y;
                    z = z + 1.0 / (1.0 + (dx * dx + dy * dy));
                }
    }
    z = wave_sum(z);
    if (row_ok && lane == 0) zrow[i] = z;
}

struct StepArgs {
    const double* P;
    int64_t ldp;
    const double* Ycur;
    double* Ynext;    // MOVE
    double* update;   // MOVE
    double* gains;    // MOVE
    double* grad;     // !MOVE: the plain gradient
    const double* zrow;
    double* klrow;    // LAST
    double* gnrow;    // LAST
    double exaggeration, momentum, lr, min_gain;
    int N;
};

template <bool LAST, bool MOVE>
__global__ __launch_bounds__(NT) void grad_kernel(StepArgs a) {
    __shared__ double2 ys[YT];
    const int N = a.N;
    const int lane = (int)threadIdx.x & 63;
    const int i = (int)blockIdx.x * ROWS + ((int)threadIdx.x >> 6);
    const bool row_ok = i < N;
    double Z = 0.0;
    for (int k = lane; k < N; k += 64) Z = Z + a.zrow[k];
    Z = wave_sum(Z);
    double2 yi = double2{0.0, 0.0};
    if (row_ok) yi = reinterpret_cast<const double2*>(a.Ycur)[i];
    const double* prow = a.P + (int64_t)(row_ok ? i : 0) * a.ldp;
    double gx = 0.0, gy = 0.0, kl = 0.0;
    for (int t0 = 0; t0 < N; t0 += YT) {
        stage_tile(a.Ycur, ys, t0, N);
        if (row_ok)
            for (int p = lane; p < YT && t0 + p < N; p += 64) {
                const int j = t0 + p;
                if (j == i) continue;
                const double dx = yi.x - ys[p].x, dy = yi.y - ys[p].y;
                const double w = 1.0 / (1.0 + (dx * dx + dy * dy));
                double q = w / Z;
                if (!(q >= EPS)) q = EPS;
                const double pe = a.exaggeration * prow[j];
                const double c = (pe - q) * w;
                gx = gx + c * dx;
                gy = gy + c * dy;
                if constexpr (LAST) kl = kl + pe * log((pe >= EPS ? pe : EPS) / q);
            }
    }
    gx = 4.0 * wave_sum(gx);
    gy = 4.0 * wave_sum(gy);
    if constexpr (LAST) kl = wave_sum(kl);
    if (!row_ok || lane != 0) return;   // (after the last barrier)
    double g[2] = {gx, gy};
    const double y[2] = {yi.x, yi.y};
    if constexpr (MOVE) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            double u = a.update[2 * (int64_t)i + c], gn = a.gains[2 * (int64_t)i + c];
            gn = (u * g[c] < 0.0) ? gn + 0.2 : gn * 0.8;
            if (gn < a.min_gain) gn = a.min_gain;
            g[c] = g[c] * gn;
            u = a.momentum * u - a.lr * g[c];
            a.update[2 * (int64_t)i + c] = u;
            a.gains[2 * (int64_t)i + c] = gn;
            a.Ynext[2 * (int64_t)i + c] = y[c] + u;
        }
    } else {
        a.grad[2 * (int64_t)i] = g[0];
        a.grad[2 * (int64_t)i + 1] = g[1];
    }
    if constexpr (LAST) {
        a.klrow[i] = kl;
        a.gnrow[i] = g[0] * g[0] + g[1] * g[1];
    }
}

__global__ __launch_bounds__(NT) void stats_kernel(const double* __restrict__ klrow, const double* __restrict__ gnrow, double* __restrict__ stats, int N) {
    __shared__ double red[NT];
    double pk = 0.0, pg = 0.0;
    for (int k = (int)threadIdx.x; k < N; k += NT) {
        pk = pk + klrow[k];
        pg = pg + gnrow[k];
    }
    const double kl = block_sum(pk, red), gn = block_sum(pg, red);
    if (threadIdx.x == 0) {
        stats[0] = kl;
        stats[1] = sqrt(gn);
    }
}

__global__ __launch_bounds__(NT) void copy_kernel(const double* __restrict__ src, double* __restrict__ dst, int n) {
    const int k = (int)blockIdx.x * NT + (int)threadIdx.x;
    if (k < n) dst[k] = src[k];
}

size_t rows_bytes(int N, int per_row) { return align_up((size_t)N * per_row * sizeof(double), 256); }

struct StepWs {
    double *yalt, *zrow, *klrow, *gnrow;
    StepWs(void* ws, int N) {
        yalt = (double*)ws;
        zrow = (double*)((char*)ws + rows_bytes(N, 2));
        klrow = (double*)((char*)zrow + rows_bytes(N, 1));
        gnrow = (double*)((char*)klrow + rows_bytes(N, 1));
    }
};

// one evaluation at a.Ycur: z partials, gradient (and the move), the statistics where asked
template <bool MOVE>
int launch_iteration(StepArgs a, const StepWs& w, bool last, double* stats, hipStream_t s) {
    const int N = a.N;
    const unsigned blocks = (unsigned)cdiv(N, ROWS);
    const double pairs = (double)N * (double)N;
    {
        ProfScope prof(s, PROF_TSNE_ZROW, N, 0, 0, 8.0 * pairs, 16.0 * (double)N * blocks);
        zrow_kernel<<<dim3(blocks), dim3(NT), 0, s>>>(a.Ycur, w.zrow, N);
        DCPT_CHECK_LAUNCH("tsne (z partials)");
    }
    {
        ProfScope prof(s, PROF_TSNE_GRAD, N, 0, 0, 20.0 * pairs, 8.0 * pairs);
        if (last) grad_kernel<true, MOVE><<<dim3(blocks), dim3(NT), 0, s>>>(a);
        else grad_kernel<false, MOVE><<<dim3(blocks), dim3(NT), 0, s>>>(a);
        DCPT_CHECK_LAUNCH("tsne (gradient)");
    }
    if (last) {
        ProfScope prof(s, PROF_TSNE_STATS, N, 0, 0, 2.0 * N, 16.0 * N);
        stats_kernel<<<dim3(1), dim3(NT), 0, s>>>(w.klrow, w.gnrow, stats, N);
        DCPT_CHECK_LAUNCH("tsne (statistics)");
    }
    return DCPT_OK;
}
}  // namespace

size_t tsne_ws_bytes(int N) { return rows_bytes(N, 2) + 3 * rows_bytes(N, 1); }

int launch_tsne_affinity_fwd(const double* d2, int64_t ldd, double* pcond, int64_t ldp, double* beta, int* steps, int N, double perplexity,
                             hipStream_t s) {
    ProfScope prof(s, PROF_TSNE_AFFINITY, N, 0, 0, 0.0, 16.0 * (double)N * (double)N);
    trace_tag("tsne.affinity");
    affinity_kernel<<<dim3((unsigned)N), dim3(NT), 0, s>>>(d2, ldd, pcond, ldp, beta, steps, N, log(perplexity));
    DCPT_CHECK_LAUNCH("tsne_affinity_fwd");
    return DCPT_OK;
}

int launch_tsne_joint_fwd(const double* pcond, int64_t ldp, double* P, int64_t ldo, void* ws, int N, hipStream_t s) {
    ProfScope prof(s, PROF_TSNE_JOINT, N, 0, 0, 0.0, 40.0 * (double)N * (double)N);
    trace_tag("tsne.joint");
    double* rs = (double*)ws;
    joint_rowsum_kernel<<<dim3((unsigned)N), dim3(NT), 0, s>>>(pcond, ldp, rs, N);
    DCPT_CHECK_LAUNCH("tsne_joint_fwd (row sums)");
    joint_kernel<<<dim3((unsigned)N), dim3(NT), 0, s>>>(pcond, ldp, P, ldo, rs, N);
    DCPT_CHECK_LAUNCH("tsne_joint_fwd");
    return DCPT_OK;
}

int launch_tsne_steps_fwd(const double* P, int64_t ldp, double* Y, double* update, double* gains, double* stats, void* ws, int N, int n_steps,
                          double exaggeration, double momentum, double lr, double min_gain, hipStream_t s) {
    trace_tag("tsne.steps");
    const StepWs w(ws, N);
    StepArgs a{};
    a.P = P; a.ldp = ldp; a.update = update; a.gains = gains; a.zrow = w.zrow; a.klrow = w.klrow; a.gnrow = w.gnrow;
    a.exaggeration = exaggeration; a.momentum = momentum; a.lr = lr; a.min_gain = min_gain; a.N = N;
    double* cur = Y;
    double* next = w.yalt;
    for (int it = 0; it < n_steps; ++it) {
        a.Ycur = cur;
        a.Ynext = next;
        DCPT_TRY(launch_iteration<true>(a, w, it == n_steps - 1, stats, s));
        double* t = cur; cur = next; next = t;
    }
    if (cur != Y) {
        copy_kernel<<<dim3((unsigned)cdiv(2 * N, NT)), dim3(NT), 0, s>>>(cur, Y, 2 * N);
        DCPT_CHECK_LAUNCH("tsne_steps_fwd (copy)");
    }
    return DCPT_OK;
}

int launch_tsne_kl_fwd(const double* P, int64_t ldp, const double* Y, double* grad, double* stats, void* ws, int N, double exaggeration,
                       hipStream_t s) {
    trace_tag("tsne.kl");
    const StepWs w(ws, N);
    StepArgs a{};
    a.P = P; a.ldp = ldp; a.Ycur = Y; a.grad = grad; a.zrow = w.zrow; a.klrow = w.klrow; a.gnrow = w.gnrow;
    a.exaggeration = exaggeration; a.N = N;
    return launch_iteration<false>(a, w, true, stats, s);
}
