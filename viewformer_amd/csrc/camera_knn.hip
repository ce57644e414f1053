// Camera k-nearest-neighbour search of the 7-Scenes pose-refinement evaluator (gfx950): for each query camera the k database cameras
// with the smallest pose distance of viewformer/evaluate/evaluate_sevenscenes.py:36-45,
//     pos_weight * ||xyz_db - xyz_q||  +  2 asin(|| vec(normalize(q_db) (x) conj(normalize(q_q))) ||),
// in ascending order, ties to the lowest index (the reference: tf.argsort over every training camera of the scene, one query at a
// time, on the host; pos_weight = 0.3).  A camera is 7 floats, xyz + quaternion (w, x, y, z).
//
// Arithmetic.  fp32, every operation explicitly rounded (no contraction) in the order of viewformer_amd/geometry.py's restatements:
// l2_normalize = x * (1 / sqrt(max(sum x^2, 1e-12))), the Hamilton product's four terms per component summed left to right, norms as
// sqrt((a^2 + b^2) + c^2).  ONE DELIBERATE DEVIATION from the reference: the asin argument is clamped to <= 1.  Rounding can put the
// norm of a unit quaternion's vector part a ulp above 1, where the reference's asin gives NaN and the row an unspecified sort position;
// here such a row gets 2 asin(1) = pi.
//
// Selection.  Distances are non-negative, so key = (float bits << 32) | index is a total order on unsigned 64-bit integers that
// sorts by distance first and index second; a NaN distance (a NaN in a database row) gets the canonical quiet-NaN bits 0x7FC00000,
// above +inf: it sorts last.  Keys are unique, so "the smallest key above the previous winner" needs no removal step, and the result
// is a pure function of the inputs: it does not depend on the tile size, the grid, how N divides, or which other queries share a call.
//   1. camera_knn_tile_kernel: one workgroup per (tile of KNN_TILE database rows, group of KNN_QG queries).  The tile is read ONCE as
//      a flat coalesced float stream into LDS (28 KB; the row stride of 7 words is odd: the per-row reads are bank-conflict free) and
//      looped over the group's queries; each thread keeps the keys of its KNN_R rows in registers, and k rounds of a workgroup-wide
//      minimum (butterfly over wave shuffles, the four waves' minima through LDS, one barrier per round: the slots alternate) emit the
//      tile's k candidates into the workspace [Q][ntiles][k].  A tile with fewer than k rows pads with ~0 keys.
//   2. knn_merge_kernel (knn_select.h, shared with code_knn.hip as are the key and the workgroup-wide minimum): one workgroup per
//      query, the same k rounds over its ntiles * k candidates.
// With a single tile (N <= KNN_TILE) the first kernel writes idx / dist itself and there is no second launch.
#include "vf_common.h"
#include "knn_select.h"
#include "../../include/vf_hip.h"

namespace {

constexpr int KNN_R = 4;                               // database rows per thread
constexpr int KNN_TILE = KNN_THREADS * KNN_R;          // database rows per workgroup

__device__ __forceinline__ float knn_sumsq3(float a, float b, float c) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(c, c));
}

// tf.math.l2_normalize's factor: rsqrt(max(sum x^2, 1e-12)) (geometry.quaternion_normalize)
__device__ __forceinline__ float knn_inv_norm4(float w, float x, float y, float z) {
    const float ss = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w, w), __fmul_rn(x, x)), __fmul_rn(y, y)), __fmul_rn(z, z));
    return __fdiv_rn(1.0f, __fsqrt_rn(fmaxf(ss, 1e-12f)));
}

struct KnnQuery {
    float x, y, z;            // position
    float w, a, b, c;         // conj(normalize(quaternion)): (w, -x, -y, -z)
};

__device__ __forceinline__ KnnQuery knn_load_query(const float* __restrict__ q) {
    KnnQuery r;
    r.x = q[0];
    r.y = q[1];
    r.z = q[2];
    const float inv = knn_inv_norm4(q[3], q[4], q[5], q[6]);
    r.w = __fmul_rn(q[3], inv);
    r.a = -__fmul_rn(q[4], inv);
    r.b = -__fmul_rn(q[5], inv);
    r.c = -__fmul_rn(q[6], inv);
    return r;
}

// distance of one database row (7 floats at p) to the query
__device__ __forceinline__ float knn_distance(const float* p, const KnnQuery& q, float pos_weight) {
    const float pos = __fsqrt_rn(knn_sumsq3(__fsub_rn(p[0], q.x), __fsub_rn(p[1], q.y), __fsub_rn(p[2], q.z)));
    const float inv = knn_inv_norm4(p[3], p[4], p[5], p[6]);
    const float w1 = __fmul_rn(p[3], inv), x1 = __fmul_rn(p[4], inv), y1 = __fmul_rn(p[5], inv), z1 = __fmul_rn(p[6], inv);
    // vector part of (w1, x1, y1, z1) (x) (q.w, q.a, q.b, q.c), term table of geometry.quaternion_multiply, summed left to right
    const float vx = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x1, q.w), __fmul_rn(y1, q.c)), -__fmul_rn(z1, q.b)), __fmul_rn(w1, q.a));
    const float vy = __fadd_rn(__fadd_rn(__fadd_rn(-__fmul_rn(x1, q.c), __fmul_rn(y1, q.w)), __fmul_rn(z1, q.a)), __fmul_rn(w1, q.b));
    const float vz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x1, q.b), -__fmul_rn(y1, q.a)), __fmul_rn(z1, q.w)), __fmul_rn(w1, q.c));
    const float s = fminf(__fsqrt_rn(knn_sumsq3(vx, vy, vz)), 1.0f);       // (fminf returns the non-NaN operand: restore a NaN below)
    const float quat = __fmul_rn(2.0f, asinf(s));
    const float d = __fadd_rn(__fmul_rn(pos, pos_weight), quat);
    return (vx != vx || vy != vy || vz != vz) ? __int_as_float(0x7FC00000) : d;
}

__global__ __launch_bounds__(KNN_THREADS) void camera_knn_tile_kernel(const float* __restrict__ db, long long N, const float* __restrict__ queries,
                                                                     int Q, int k, float pos_weight, int ntiles,
                                                                     unsigned long long* __restrict__ cand, int32_t* __restrict__ idx,
                                                                     float* __restrict__ dist) {
    __shared__ float rows[KNN_TILE * 7];
    __shared__ unsigned long long red[2][KNN_WAVES];
    const int tid = threadIdx.x;
    const long long tile = blockIdx.x, row0 = tile * KNN_TILE;
    const int nrows = (int)(N - row0 < KNN_TILE ? N - row0 : KNN_TILE);
    const float* src = db + row0 * 7;
    for (int i = tid; i < nrows * 7; i += KNN_THREADS) rows[i] = src[i];
    __syncthreads();

    const int q0 = blockIdx.y * KNN_QG, q1 = q0 + KNN_QG < Q ? q0 + KNN_QG : Q;
    unsigned round = 0;
    for (int q = q0; q < q1; ++q) {
        const KnnQuery qq = knn_load_query(queries + (long long)q * 7);
        unsigned long long key[KNN_R];
#pragma unroll
        for (int j = 0; j < KNN_R; ++j) {
            const int r = tid + j * KNN_THREADS;
            key[j] = r < nrows ? knn_key(knn_distance(rows + r * 7, qq, pos_weight), (unsigned)(row0 + r)) : KNN_NONE;
        }
        unsigned long long lower = 0;                       // candidates of a round: the keys >= lower (= the last winner + 1)
        for (int r = 0; r < k; ++r, ++round) {
            unsigned long long m = KNN_NONE;
#pragma unroll
            for (int j = 0; j < KNN_R; ++j) m = knn_min(m, key[j] >= lower ? key[j] : KNN_NONE);
            m = knn_block_min(m, red[round & 1]);
            if (tid == 0) {
                if (ntiles == 1) knn_emit(m, idx, dist, (long long)q * k + r);      // (N >= k: a single tile always holds k rows)
                else cand[((long long)q * ntiles + tile) * k + r] = m;
            }
            lower = m == KNN_NONE ? KNN_NONE : m + 1;
        }
    }
}

bool knn_shape_ok(int64_t N, int Q, int k) { return k >= 1 && k <= KNN_MAX_K && N >= k && N <= 0x7fffffffll && Q >= 0; }

long long knn_tiles(int64_t N) { return (N + KNN_TILE - 1) / KNN_TILE; }

}  // namespace

extern "C" {

size_t vf_camera_knn_workspace_bytes(int64_t N, int Q, int k) {
    if (!knn_shape_ok(N, Q, k)) return 0;
    const long long ntiles = knn_tiles(N);
    if (ntiles == 1) return 0;
    return (size_t)Q * (size_t)ntiles * (size_t)k * sizeof(unsigned long long);
}

int vf_camera_knn_f32(const float* db, int64_t N, const float* queries, int Q, int k, float pos_weight, int32_t* idx, float* dist,
                      void* workspace, void* stream) {
    if (k < 1 || N < k || Q < 0 || !(pos_weight >= 0.0f && pos_weight < __builtin_inff())) return VF_ERR_BAD_ARG;
    if (k > KNN_MAX_K || N > 0x7fffffffll) return VF_ERR_UNSUPPORTED;
    if (Q == 0) return VF_OK;
    const long long ntiles = knn_tiles(N);
    if (!db || !queries || !idx || (ntiles > 1 && !workspace)) return VF_ERR_BAD_ARG;
    if ((uintptr_t)workspace & 7) return VF_ERR_BAD_ARG;
    const int qgroups = (Q + KNN_QG - 1) / KNN_QG;
    if (qgroups > 65535) return VF_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* cand = (unsigned long long*)workspace;
    hipLaunchKernelGGL(camera_knn_tile_kernel, dim3((unsigned)ntiles, (unsigned)qgroups), dim3(KNN_THREADS), 0, s, db, (long long)N, queries,
                       Q, k, pos_weight, (int)ntiles, cand, idx, dist);
    if (ntiles > 1)
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)Q), dim3(KNN_THREADS), 0, s, cand, ntiles * k, k, idx, dist);
    return vf_last_status();
}

}  // extern "C"
