// The mean of the distribution vf_sample_rows_f32 draws from, in the codebook's latent space: out[d] = sum_n p_n E[d][n], gfx950.
//
// Per row z[0..N) with T > 0, top_k >= 0, top_p > 0 (include/vf_hip.h has the full contract):
//   1. the kept set is the sampler's, steps (1)-(3) there: row_filter.h's vf_row_filter, the routine sample_rows.hip runs, so kept and thr
//      are the sampler's bits by construction;
//   2. p_n = e_n / sum_kept e for the kept n, e_n = e^((z_n - max z) / T) by vf_exp_neg; every other code has p_n = +0;
//   3. out[d] = sum_n p_n E[d][n]: fp32 products and sums on v_mfma_f32_16x16x4_f32 (an fmaf chain, bit for bit), codes ascending — ONE
//      chain per output element, started at +0;
//   4. a row without a finite logit: kept 0, thr NaN, out all NaN.
//
// One workgroup of 4 waves per R = 16 rows.
//   Phase 1: wave w filters the rows 4 w ... 4 w + 3, one after the other, and parks p as fp32 in LDS, P[16][ldP] (ldP = N rounded up to 64,
//            plus 4: the MFMA's B-operand reads, 16 rows x 4 codes, then touch 64 different banks).  Rows past the end hold zeros.
//   Phase 2: out^T [D x 16] = E [D x N] . P^T [N x 16].  Wave w owns the feature tiles (16 features each) w, w + 4, ...; the codes are walked
//            in tiles of 32, E's tile [D][32] staged through LDS (two buffers, rows 36 floats apart: the A-operand reads are conflict-free) and
//            shared by the 16 rows.  A code tile that none of the 16 rows keeps is skipped: its p are +0 in every row and E is finite (the
//            caller's contract), so it would add an exact zero to accumulators that started at +0 — skipping cannot change a bit, and the
//            tiles that remain are still walked in ascending order.  That is what makes a nucleus (top_p = 0.9) cheap.
// A row's chain is therefore the same alone or among others, at any position in its workgroup and whatever the other rows keep.
// No atomics; exactly rows x D elements of out and rows of kept / thr are written; columns >= N of the logits and of E are never read.
#include "vf_common.h"
#include "row_filter.h"
#include "../../include/vf_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MIX_R = 16;           // rows per workgroup = the MFMA's 16 columns
constexpr int MIX_TILE = 32;        // codes per staged tile of E
constexpr int MIX_LDT = 36;         // floats between two features of a staged tile
constexpr int MIX_MAX_N = 1024, MIX_MAX_D = 256;

__host__ __device__ constexpr int mix_ldp(int n) { return (n + 63) / 64 * 64 + 4; }

__global__ __launch_bounds__(256) void mix_rows_kernel(const float* __restrict__ x, long long rows, int n, long long ld, float T, int top_k,
                                                       float top_p, const float* __restrict__ E, int D, long long ldE, float* __restrict__ out,
                                                       long long ldo, int* __restrict__ kept_out, float* __restrict__ thr_out) {
    extern __shared__ float lds[];
    __shared__ uint32_t s_tiles[4];
    __shared__ int s_empty[MIX_R];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ldP = mix_ldp(n);
    const int npad = (n + MIX_TILE - 1) / MIX_TILE * MIX_TILE;
    float* P = lds;
    float* Et = lds + MIX_R * ldP;                                           // [2][D][MIX_LDT]

    // ---- phase 1: the kept set and p of this wave's four rows
    uint32_t wtiles = 0;                                                     // bit i: one of this wave's rows keeps a code of tile i
    for (int i = 0; i < 4; ++i) {
        const int rl = w * 4 + i;
        const long long row = (long long)blockIdx.x * MIX_R + rl;
        float* pr = P + rl * ldP;
        bool live = false, empty = false;
        if (row < rows) {                                                   // a whole wave
            uint32_t kimg[16];
            float dd[16], ee[16];
            float zmax, mass;
            uint32_t t;
            live = vf_row_filter<true>(x + (size_t)row * ld, n, lane, T, top_k, top_p, kimg, dd, ee, zmax, t, mass);
            empty = !live;
            if (live) {
                int cnt = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int c = lane + 64 * j;
                    const bool keep = kimg[j] >= t;
                    const unsigned long long b = __ballot(keep);
                    cnt += __popcll(b);
                    wtiles |= ((b & 0xFFFFFFFFull) ? 1u : 0u) << (2 * j) | ((b >> 32) ? 1u : 0u) << (2 * j + 1);
                    if (c < npad) pr[c] = keep ? __fdiv_rn(ee[j], mass) : 0.0f;
                }
                if (lane == 0) {
                    if (kept_out) kept_out[row] = cnt;
                    if (thr_out) thr_out[row] = __fdiv_rn(vf_img_inv(t), T);
                }
            } else if (lane == 0) {
                if (kept_out) kept_out[row] = 0;
                if (thr_out) thr_out[row] = __builtin_nanf("");
            }
        }
        if (!live)
            for (int c = lane; c < npad; c += 64) pr[c] = 0.0f;
        if (lane == 0) s_empty[rl] = empty;
    }
    if (lane == 0) s_tiles[w] = wtiles;
    __syncthreads();
    const uint32_t tiles = s_tiles[0] | s_tiles[1] | s_tiles[2] | s_tiles[3];

    // ---- phase 2: out^T = E . P^T over the kept tiles, ascending
    const int MT = D >> 4;                                                   // feature tiles; this wave's: w, w + 4, w + 8, w + 12
    const int l15 = lane & 15, l4 = lane >> 4;
    f32x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (tiles) {
        const int cc = threadIdx.x & 31, dr = threadIdx.x >> 5;              // staging: thread -> code cc of the tile, features dr + 8 i
        float stage[MIX_MAX_D / 8];
        int cur = __ffs((int)tiles) - 1;
        auto fetch = [&](int tile) {
            const int c = tile * MIX_TILE + cc;
#pragma unroll
            for (int i = 0; i < MIX_MAX_D / 8; ++i) {
                const int d = dr + 8 * i;
                stage[i] = (d < D && c < n) ? E[(size_t)d * ldE + c] : 0.0f;
            }
        };
        auto park = [&](int buf) {
            float* dst = Et + (size_t)buf * D * MIX_LDT;
#pragma unroll
            for (int i = 0; i < MIX_MAX_D / 8; ++i) {
                const int d = dr + 8 * i;
                if (d < D) dst[d * MIX_LDT + cc] = stage[i];
            }
        };
        fetch(cur);
        park(0);
        __syncthreads();
        int buf = 0;
        while (true) {
            const uint32_t rest = tiles & ~((2u << cur) - 1u);
            const int next = rest ? __ffs((int)rest) - 1 : -1;
            if (next >= 0) fetch(next);
            const float* et = Et + (size_t)buf * D * MIX_LDT;
            const float* pb = P + l15 * ldP + cur * MIX_TILE + l4;
#pragma unroll
            for (int k0 = 0; k0 < MIX_TILE; k0 += 4) {
                const float b = pb[k0];                                      // B[k = lane >> 4][column = lane & 15] = p of row l15, code k0 + l4
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int mt = w + 4 * m;
                    if (mt < MT) {                                          // (uniform over the wave)
                        const float a = et[(mt * 16 + l15) * MIX_LDT + k0 + l4];       // A[feature = lane & 15][k = lane >> 4]
                        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[m], 0, 0, 0);
                    }
                }
            }
            if (next < 0) break;
            park(buf ^ 1);
            __syncthreads();
            buf ^= 1;
            cur = next;
        }
    }

    // ---- the results: lane holds the features mt 16 + 4 (lane >> 4) + r, r < 4, of row lane & 15
    const long long row = (long long)blockIdx.x * MIX_R + l15;
    if (row < rows) {
        const bool empty = s_empty[l15] != 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int mt = w + 4 * m;
            if (mt < MT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(size_t)row * ldo + mt * 16 + l4 * 4 + r] = empty ? __builtin_nanf("") : acc[m][r];
            }
        }
    }
}

}  // namespace

extern "C" {

int vf_mix_rows_f32(const float* logits, int64_t rows, int N, int64_t ld, float temperature, int top_k, float top_p, const float* E, int D,
                    int64_t ldE, float* out, int64_t ldo, int32_t* kept, float* thr, void* stream) {
    if (!logits || !E || !out || rows < 0 || N < 1 || ld < N || ldE < N || D < 1 || ldo < D) return VF_ERR_BAD_ARG;
    if (!(temperature > 0.f) || !(temperature <= 3.402823466e38f)) return VF_ERR_BAD_ARG;      // <= 0, NaN, inf
    if (!(top_p > 0.f) || top_k < 0) return VF_ERR_BAD_ARG;
    if (N > MIX_MAX_N || D % 32 != 0 || D > MIX_MAX_D || rows > 0x7fffffffLL * MIX_R) return VF_ERR_UNSUPPORTED;
    if (rows == 0) return VF_OK;
    const size_t smem = ((size_t)MIX_R * mix_ldp(N) + 2 * (size_t)D * MIX_LDT) * sizeof(float);
    static unsigned long long attr_devs = 0;      // bit d: raised on device d (the attribute is per device)
    if (vf_attr_needed(&attr_devs)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mix_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(((size_t)MIX_R * mix_ldp(MIX_MAX_N) + 2 * (size_t)MIX_MAX_D * MIX_LDT) * sizeof(float)));
        if (e != hipSuccess) return (int)e;
        vf_attr_done(&attr_devs);
    }
    hipLaunchKernelGGL(mix_rows_kernel, dim3((unsigned)((rows + MIX_R - 1) / MIX_R)), dim3(256), smem, (hipStream_t)stream, logits,
                       (long long)rows, N, (long long)ld, temperature, top_k, top_p, E, D, (long long)ldE, out, (long long)ldo,
                       reinterpret_cast<int*>(kept), thr);
    return vf_last_status();
}

}  // extern "C"
