// Exact, order-independent top-k selection shared by the k-nearest-neighbour kernels (camera_knn.hip, code_knn.hip).
//
// Distances are non-negative, so key = (float bits << 32) | index is a total order on unsigned 64-bit integers that sorts by distance
// first and index second; a NaN distance gets the canonical quiet-NaN bits 0x7FC00000, above +inf: it sorts last.  Keys are unique, so
// "the smallest key above the previous winner" needs no removal step, and the result is a pure function of the keys: it does not depend
// on the tile size, the grid, how N divides, or which other queries share a call.  A tile kernel emits its tile's k smallest keys into
// a workspace [Q][ntiles][k] (~0 where the tile has fewer than k rows); knn_merge_kernel, one workgroup per query, runs the same k
// rounds over the query's ntiles * k candidates.
#pragma once
#include "vf_common.h"

namespace {

constexpr int KNN_THREADS = 256;
constexpr int KNN_WAVES = KNN_THREADS / VF_WAVE;
constexpr int KNN_QG = 8;                              // queries per workgroup of a tile kernel
constexpr int KNN_MAX_K = 32;
constexpr unsigned long long KNN_NONE = ~0ull;

__device__ __forceinline__ unsigned long long knn_key(float d, unsigned index) {
    const unsigned bits = d != d ? 0x7FC00000u : __float_as_uint(d);
    return ((unsigned long long)bits << 32) | index;
}

__device__ __forceinline__ unsigned long long knn_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// workgroup-wide minimum: butterfly inside each wave, the waves' minima through `slot` (KNN_WAVES words), ONE barrier.  The caller
// alternates between two slots from round to round, so a wave that is already in the next round cannot overwrite what a slower wave
// still reads.
__device__ __forceinline__ unsigned long long knn_block_min(unsigned long long m, unsigned long long* slot) {
#pragma unroll
    for (int o = VF_WAVE / 2; o > 0; o >>= 1) m = knn_min(m, __shfl_xor(m, o, VF_WAVE));
    if ((threadIdx.x & (VF_WAVE - 1)) == 0) slot[threadIdx.x / VF_WAVE] = m;
    __syncthreads();
    unsigned long long r = slot[0];
#pragma unroll
    for (int w = 1; w < KNN_WAVES; ++w) r = knn_min(r, slot[w]);
    return r;
}

__device__ __forceinline__ void knn_emit(unsigned long long key, int32_t* __restrict__ idx, float* __restrict__ dist, long long at) {
    idx[at] = (int32_t)(unsigned)key;
    if (dist) dist[at] = __uint_as_float((unsigned)(key >> 32));
}

__global__ __launch_bounds__(KNN_THREADS) void knn_merge_kernel(const unsigned long long* __restrict__ cand, long long n, int k,
                                                               int32_t* __restrict__ idx, float* __restrict__ dist) {
    __shared__ unsigned long long red[2][KNN_WAVES];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const unsigned long long* c = cand + q * n;
    unsigned long long lower = 0;
    for (int r = 0; r < k; ++r) {
        unsigned long long m = KNN_NONE;
        for (long long i = tid; i < n; i += KNN_THREADS) {
            const unsigned long long v = c[i];
            m = knn_min(m, v >= lower ? v : KNN_NONE);
        }
        m = knn_block_min(m, red[r & 1]);
        if (tid == 0) knn_emit(m, idx, dist, q * k + r);
        lower = m == KNN_NONE ? KNN_NONE : m + 1;
    }
}

}  // namespace
