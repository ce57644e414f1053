// Image retrieval on VQ codes (gfx950): the distance table of a codebook, and for each query photo's code map the k database code maps
// with the smallest windowed one-sided Chamfer distance
//     T[a][b]  = || e_a - e_b ||^2                                   (e_c: the codebook's embedding of code c)
//     d_w(q,m) = sum_p  min_{p' in W_w(p)}  T[q[p]][m[p']]           (p over the t x t token grid; W_w(p): the positions within Chebyshev
//                                                                     distance w of p, clipped at the grid's border)
// in ascending order, ties to the lowest index.  w = 0 is the squared L2 distance between the two photos' quantised latent maps, computed
// without touching a pixel or a latent; w = t - 1 is the full one-sided Chamfer distance.  (The reference reads its image matches from a
// text file made by an outside retrieval system, viewformer/evaluate/evaluate_sevenscenes.py:71-77; this is the search that makes such a
// file from a scene_bank.SceneBank.)
//
// Arithmetic.  fp32, every operation explicitly rounded, no contraction.  Table: T[a][b] = sum_j fl(fl(e_a[j] - e_b[j])^2), j ascending
// from 0: exactly symmetric and exactly 0 on the diagonal for finite embeddings.  Distance: the inner minimum starts at +inf and takes a
// candidate iff candidate < current (a NaN table entry never enters); the outer sum runs over p ascending, starting from the first term.
// A query code outside [0, K) makes its term +inf; a database code outside [0, K) is skipped as a candidate.  The table is never read
// out of bounds: codes are range-checked where they are staged, and every invalid code is redirected to an extra +inf entry behind each
// staged table row.
//
//   1. codebook_dist_table_kernel: one thread per (4 rows a, 1 column b); a's are uniform over a wave (broadcast loads), b's coalesced.
//   2. code_knn_tile_kernel: one workgroup per (tile of CK_TILE database rows, group of KNN_QG queries), one database row per thread.  The
//      tile's codes are read ONCE, coalesced, into LDS as 16-bit values, position-major [t*t][CK_TILE + 2] (the odd dword stride makes
//      the transposing store conflict-free; a thread's reads of position p' sit next to its neighbours').  Per query the table rows
//      T[q[p]][.] are uniform over the workgroup: they are staged into LDS in chunks of consecutive positions p (K + 1 floats each, the
//      last one +inf), and every thread gathers from them with its own row's codes.  Chunking by p keeps the order of additions.  Then
//      the k rounds of knn_select.h emit the tile's k candidates (or, with a single tile, idx / dist themselves).
//   3. knn_merge_kernel (knn_select.h): one workgroup per query over its ntiles * k candidates.
#include "vf_common.h"
#include "knn_select.h"
#include "../../include/vf_hip.h"

// hipcc contracts a * b + c into one fma by default, and through __fmul_rn / __fadd_rn as well (plain operators compiled under the
// header's own setting, inlined with it): the table's fl(acc + fl(d * d)) needs both roundings, so the rounded operations of this file
// are its own, compiled with contraction off
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float ck_sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float ck_mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float ck_add_rn(float a, float b) { return a + b; }

constexpr int CK_TILE = KNN_THREADS;                   // database rows per workgroup: one per thread
constexpr int CK_CODE_LD = CK_TILE + 2;                // 16-bit codes per position in LDS: 129 dwords
constexpr int CK_MAX_T = 16;
constexpr int CK_MAX_K = 4096;
constexpr int CK_ROWS_BYTES = 8 * (1024 + 1) * 4;      // staged table rows per chunk: 8 positions at K = 1024
constexpr int CK_STAGE = 8;                            // table rows staged per pass
constexpr int CK_LDS_BYTES = 160 * 1024 - 64;          // the CU's LDS less the selection's static slots

__global__ __launch_bounds__(256) void codebook_dist_table_kernel(const float* __restrict__ E, int D, int K, long long ldE,
                                                                 float* __restrict__ table) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int a0 = (blockIdx.y * 4 + threadIdx.y) * 4;
    if (b >= K || a0 >= K) return;
    int a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = a0 + i < K ? a0 + i : K - 1;            // (clamped rows are computed and not stored)
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < D; ++j) {
        const float* e = E + j * ldE;
        const float eb = e[b];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = ck_sub_rn(e[a[i]], eb);
            acc[i] = ck_add_rn(acc[i], ck_mul_rn(d, d));
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (a0 + i < K) table[(long long)(a0 + i) * K + b] = acc[i];
}

__global__ __launch_bounds__(KNN_THREADS) void code_knn_tile_kernel(const int32_t* __restrict__ db, long long N, long long ld_db,
                                                                   const int32_t* __restrict__ queries, int Q, long long ld_q, int t,
                                                                   const float* __restrict__ table, int K, int window,
                                                                   const int32_t* __restrict__ exclude, int k, int ntiles, int chunk,
                                                                   unsigned long long* __restrict__ cand, int32_t* __restrict__ idx,
                                                                   float* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ck_smem[];
    __shared__ unsigned long long red[2][KNN_WAVES];
    const int tid = threadIdx.x;
    const int P = t * t, KS = K + 1;
    unsigned short* codes = reinterpret_cast<unsigned short*>(ck_smem);                        // [P][CK_CODE_LD]
    float* rows = reinterpret_cast<float*>(ck_smem + (size_t)P * CK_CODE_LD * sizeof(unsigned short));   // [chunk][KS]
    const float inf = __builtin_inff();

    const long long tile = blockIdx.x, row0 = tile * CK_TILE;
    const int nrows = (int)(N - row0 < CK_TILE ? N - row0 : CK_TILE);
    for (int i = tid; i < CK_TILE * P; i += KNN_THREADS) {
        const int r = i / P, p = i - r * P;
        int c = K;                                                                            // rows beyond N and codes outside [0, K): the +inf entry
        if (r < nrows) {
            const int32_t v = db[(row0 + r) * ld_db + p];
            if ((unsigned)v < (unsigned)K) c = v;
        }
        codes[p * CK_CODE_LD + r] = (unsigned short)c;
    }

    const int q0 = blockIdx.y * KNN_QG, q1 = q0 + KNN_QG < Q ? q0 + KNN_QG : Q;
    unsigned round = 0;
    for (int q = q0; q < q1; ++q) {
        const int32_t* qc = queries + q * ld_q;
        float acc = 0.0f;
        for (int p0 = 0; p0 < P; p0 += chunk) {
            const int pc = P - p0 < chunk ? P - p0 : chunk;
            __syncthreads();                                                                  // the tile's codes are in place; the last chunk's readers are done
            for (int c0 = 0; c0 < pc; c0 += CK_STAGE) {                                       // CK_STAGE rows at a time: their loads are in flight together
                const float* src[CK_STAGE];
#pragma unroll
                for (int u = 0; u < CK_STAGE; ++u) {
                    const int32_t v = c0 + u < pc ? qc[p0 + c0 + u] : -1;
                    src[u] = (unsigned)v < (unsigned)K ? table + (long long)v * K : nullptr;   // (an invalid query code: a row of +inf)
                }
#pragma unroll 4
                for (int i = tid; i < KS; i += KNN_THREADS) {
                    float v[CK_STAGE];
#pragma unroll
                    for (int u = 0; u < CK_STAGE; ++u) v[u] = src[u] && i < K ? src[u][i] : inf;
#pragma unroll
                    for (int u = 0; u < CK_STAGE; ++u)
                        if (c0 + u < pc) rows[(c0 + u) * KS + i] = v[u];
                }
            }
            __syncthreads();
            for (int c = 0; c < pc; ++c) {
                const int p = p0 + c, py = p / t, px = p - py * t;
                const int y0 = py - window > 0 ? py - window : 0, y1 = py + window < t - 1 ? py + window : t - 1;
                const int x0 = px - window > 0 ? px - window : 0, x1 = px + window < t - 1 ? px + window : t - 1;
                const float* row = rows + c * KS;
                float m = inf;
                for (int y = y0; y <= y1; ++y)
                    for (int x = x0; x <= x1; x += 4) {                                       // four gathers in flight; past the window's end
                        float v[4];                                                          // the last candidate again: the minimum does not mind
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int xx = x + u < x1 ? x + u : x1;
                            v[u] = row[codes[(y * t + xx) * CK_CODE_LD + tid]];
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) m = v[u] < m ? v[u] : m;
                    }
                acc = p == 0 ? m : ck_add_rn(acc, m);
            }
        }
        const long long me = row0 + tid;
        const long long skip = exclude ? (long long)exclude[q] : -1;
        const unsigned long long key = tid < nrows && me != skip ? knn_key(acc, (unsigned)me) : KNN_NONE;
        unsigned long long lower = 0;                       // candidates of a round: the keys >= lower (= the last winner + 1)
        for (int r = 0; r < k; ++r, ++round) {
            unsigned long long m = knn_block_min(key >= lower ? key : KNN_NONE, red[round & 1]);
            if (tid == 0) {
                if (ntiles == 1) knn_emit(m, idx, dist, (long long)q * k + r);      // (N - 1 >= k: a single tile always holds k rows)
                else cand[((long long)q * ntiles + tile) * k + r] = m;
            }
            lower = m == KNN_NONE ? KNN_NONE : m + 1;
        }
    }
}

bool ck_shape_ok(int64_t N, int Q, int k) { return k >= 1 && k <= KNN_MAX_K && N >= k && N <= 0x7fffffffll && Q >= 0; }

long long ck_tiles(int64_t N) { return (N + CK_TILE - 1) / CK_TILE; }

bool ck_misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" {

int vf_codebook_dist_table_f32(const float* E, int D, int K, int64_t ldE, float* table, void* stream) {
    if (!E || !table || ck_misaligned(E, 3) || ck_misaligned(table, 3) || ldE < K) return VF_ERR_BAD_ARG;
    if (K < 1 || K > CK_MAX_K || D < 1) return VF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(codebook_dist_table_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)((K + 15) / 16)), dim3(64, 4), 0,
                       (hipStream_t)stream, E, D, K, (long long)ldE, table);
    return vf_last_status();
}

size_t vf_code_knn_workspace_bytes(int64_t N, int Q, int k) {
    if (!ck_shape_ok(N, Q, k)) return 0;
    const long long ntiles = ck_tiles(N);
    if (ntiles == 1) return 0;
    return (size_t)Q * (size_t)ntiles * (size_t)k * sizeof(unsigned long long);
}

int vf_code_knn_f32(const int32_t* db, int64_t N, int64_t ld_db, const int32_t* queries, int Q, int64_t ld_q, int t, const float* table,
                    int K, int window, const int32_t* exclude, int k, int32_t* idx, float* dist, void* workspace, void* stream) {
    if (k < 1 || N < (int64_t)k + (exclude ? 1 : 0) || Q < 0 || t < 1 || K < 1 || window < 0) return VF_ERR_BAD_ARG;
    if (k > KNN_MAX_K || N > 0x7fffffffll || t > CK_MAX_T || K > CK_MAX_K) return VF_ERR_UNSUPPORTED;
    if (window > t - 1 || ld_db < t * t || ld_q < t * t) return VF_ERR_BAD_ARG;
    if (Q == 0) return VF_OK;
    const long long ntiles = ck_tiles(N);
    if (!db || !queries || !table || !idx || (ntiles > 1 && !workspace)) return VF_ERR_BAD_ARG;
    if (ck_misaligned(db, 3) || ck_misaligned(queries, 3) || ck_misaligned(table, 3) || ck_misaligned(exclude, 3) || ck_misaligned(idx, 3) ||
        ck_misaligned(dist, 3) || ck_misaligned(workspace, 7))
        return VF_ERR_BAD_ARG;
    const int qgroups = (Q + KNN_QG - 1) / KNN_QG;
    if (qgroups > 65535) return VF_ERR_UNSUPPORTED;
    // LDS: the tile's codes, then as many staged table rows as CK_ROWS_BYTES (and the CU) hold, at least one: 132 096 + 16 388 bytes at
    // t = 16, K = 4096
    const int P = t * t;
    const size_t code_bytes = (size_t)P * CK_CODE_LD * sizeof(unsigned short), row_bytes = (size_t)(K + 1) * sizeof(float);
    const size_t budget = CK_LDS_BYTES - code_bytes < (size_t)CK_ROWS_BYTES ? CK_LDS_BYTES - code_bytes : (size_t)CK_ROWS_BYTES;
    int chunk = (int)(budget / row_bytes);
    chunk = chunk < 1 ? 1 : chunk > P ? P : chunk;
    const size_t smem = code_bytes + chunk * row_bytes;
    static unsigned long long attr_devs = 0;
    if (smem > 64 * 1024 && vf_attr_needed(&attr_devs)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(code_knn_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 CK_LDS_BYTES);
        if (e != hipSuccess) return (int)e;
        vf_attr_done(&attr_devs);
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* cand = (unsigned long long*)workspace;
    hipLaunchKernelGGL(code_knn_tile_kernel, dim3((unsigned)ntiles, (unsigned)qgroups), dim3(KNN_THREADS), smem, s, db, (long long)N,
                       (long long)ld_db, queries, Q, (long long)ld_q, t, table, K, window, exclude, k, (int)ntiles, chunk, cand, idx, dist);
    if (ntiles > 1) hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)Q), dim3(KNN_THREADS), 0, s, cand, ntiles * k, k, idx, dist);
    return vf_last_status();
}

}  // extern "C"
