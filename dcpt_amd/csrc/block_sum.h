// The fixed-order sums of the fp64 kernels (metrics.hip, metrics_ms.hip, ssim_loss.hip, ldl.hip, tsne.hip): the binary tree over the 256
// threads of a workgroup, and the kernel that adds a group's per-workgroup partials in that order.  No atomics anywhere, so the same input
// gives the same bits on every run.  Nothing here multiplies into a sum, so nothing here depends on the including file's contraction setting.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dcpt_common.h"

namespace {
constexpr int BLOCK_NT = 256;   // threads per workgroup of every kernel that uses the tree

// red[t] = op(red[t], red[t + s]) for s = 128, 64, ... 1; every thread returns the result, and `red` may be reused at once
template <typename T, typename Op>
__device__ __forceinline__ T block_tree(T v, T* red, Op op) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = BLOCK_NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = op(red[tid], red[tid + s]);
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    return block_tree(v, red, [](T a, T b) { return a + b; });
}

// what the reduce kernel stores: the sum, sum / N (a mean), sqrt(sum / (N - 1)) (the unbiased std from a sum of squared deviations)
enum { SUM_PLAIN, SUM_MEAN, SUM_STD };

// out[g][j] = the sum over i < n of part[g][i][j], j < nj, finished as MODE says: one workgroup per group g, thread t adds i = t, t + 256, ...
// in ascending order, then the tree
template <int MODE>
__global__ __launch_bounds__(BLOCK_NT) void sum_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int64_t n, int nj,
                                                              int64_t N) {
    __shared__ double red[BLOCK_NT];
    const int tid = threadIdx.x;
    const double* p = part + (int64_t)blockIdx.x * n * nj;
    for (int j = 0; j < nj; ++j) {
        double a = 0.0;
        for (int64_t i = tid; i < n; i += BLOCK_NT) a += p[i * nj + j];
        a = block_sum(a, red);
        if (tid == 0) out[(int64_t)blockIdx.x * nj + j] = MODE == SUM_MEAN ? a / (double)N : (MODE == SUM_STD ? sqrt(a / (double)(N - 1)) : a);
    }
}
}  // namespace
