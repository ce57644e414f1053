// Draw codes from rows of logits: temperature, top-k, top-p (nucleus) and S reproducible draws per row in one launch, gfx950.
//
// A MASK view's tokens are independent given the context, so S samples of a view are S draws from each row of ONE set of logits.  Per row
// z[0..N), with T > 0, top_k >= 0, top_p > 0, a seed, a 64-bit row_id and the sample index s (include/vf_hip.h has the full contract):
//   1. y_n = z_n / T; a -inf logit has probability 0 and is never kept; a row without a finite logit gives idx -1, logp NaN, kept 0.
//   2. top-k: keep {n : y_n >= the k-th largest value} (ties at that value all kept); skipped for k = 0 or k >= the number of finite logits.
//   3. top-p on what 2. left: with e_n = e^(y_n - max y), keep {n : y_n >= v*}, v* the largest value of the row whose mass
//      sum_{kept, y_n >= v} e_n reaches top_p x the mass of everything 2. left; skipped for top_p >= 1.  The maximum is always kept.
//   4. noise: key = vf_dropout_hash(seed, 0x5A0000 + s, row_id), w_n = lowbias32(n ^ key), u_n = ((w_n >> 9) + 0.5) 2^-23,
//      g_n = -log(-log u_n)                                                  (viewformer_amd/_hash.py restates it)
//   5. idx = arg-max over the kept n of y_n + g_n, lowest index on equal keys (Gumbel-max: an exact draw from the soft-max of the kept set)
//   6. logp = y_idx - (max y + log sum_kept e_n)
//
// One wave per row.  The kept set — the read, d and e once per row, the bitwise threshold searches on the order-preserving integer image of
// the logits — is row_filter.h's vf_row_filter, shared with mix_rows.hip; the draws below walk the same registers with its VF_ROW_FOR.
//
// The key of the arg-max is d_n + g_n, not y_n + g_n: the same arg-max in exact arithmetic (a shift by max y), without |max y| in the
// rounding of the sum; logp = d_idx - log(sum_kept e) likewise.  -log u is formed as -log1p(-(1 - u)): 1 - u is exact in fp32 and the
// winners are the codes with u close to 1, where a plain fp32 log of u loses its relative accuracy.
//
// A row's outputs depend on its logits, the parameters, seed and row_id only: not on rows, on where the row sits, on ld, on S (sample s of
// any launch is sample s) or on the optional outputs requested.
#include "vf_common.h"
#include "row_filter.h"
#include "../../include/vf_hip.h"

namespace {

constexpr uint32_t SITE_SAMPLE = 0x5A0000u;

// g = -log(-log u), u = ((w >> 9) + 0.5) 2^-23 in (0, 1): 1 - u is exact, -log u = -log1p(-(1 - u))
__device__ __forceinline__ float gumbel_of(uint32_t w) {
    const float u = __fmul_rn(__fadd_rn((float)(w >> 9), 0.5f), 1.1920928955078125e-7f);
    const float a = __fsub_rn(1.0f, u);
    return -logf(-log1pf(-a));
}

template <bool REG>
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ x, long long rows, int n, long long ld, float T, int top_k,
                                                          float top_p, uint32_t seed, const long long* __restrict__ row_id, int S,
                                                          long long* __restrict__ idx_out, float* __restrict__ logp_out,
                                                          int* __restrict__ kept_out, float* __restrict__ thr_out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                // a whole wave
    const float* xr = x + (size_t)row * ld;
    const uint64_t rid = row_id ? (uint64_t)row_id[row] : (uint64_t)row;

    // ---- the kept set: its threshold's image t and its mass (row_filter.h)
    uint32_t kimg[16];
    float dd[16], ee[16];
    float zmax, mass;
    uint32_t t;
    if (!vf_row_filter<REG>(xr, n, lane, T, top_k, top_p, kimg, dd, ee, zmax, t, mass)) {      // no finite logit: no distribution
        for (int s = lane; s < S; s += 64) {
            idx_out[(size_t)row * S + s] = -1;
            if (logp_out) logp_out[(size_t)row * S + s] = __builtin_nanf("");
        }
        if (lane == 0) {
            if (kept_out) kept_out[row] = 0;
            if (thr_out) thr_out[row] = __builtin_nanf("");
        }
        return;
    }
    const float lsum = logf(mass);                                           // mass >= 1: the maximum's e is exactly 1
    if (kept_out || thr_out) {
        int cnt = 0;
        VF_ROW_FOR(cnt += __popcll(__ballot(k >= t));)
        if (lane == 0) {
            if (kept_out) kept_out[row] = cnt;
            if (thr_out) thr_out[row] = __fdiv_rn(vf_img_inv(t), T);
        }
    }

    // ---- the draws: Gumbel-max over the kept set, first index on equal keys
    long long my_idx = 0;
    float my_lp = 0.f;
    for (int s = 0; s < S; ++s) {
        const uint32_t key = vf_dropout_hash(seed, SITE_SAMPLE + (uint32_t)s, rid);
        float bv = -INFINITY, bd = 0.f;
        int bi = 0x7fffffff;
        VF_ROW_FOR(
            if (__ballot(k >= t)) {                                          // (a slot that holds no kept code in any lane costs nothing)
                const float v = k >= t ? __fadd_rn(d, gumbel_of(vf_lowbias32((uint32_t)c ^ key))) : -INFINITY;
                if (v > bv) { bv = v; bi = c; bd = d; }                      // strict: the first maximum of this lane's (ascending) columns
            })
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64), od = __shfl_xor(bd, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; bd = od; }
        }
        if ((s & 63) == lane) {
            my_idx = bi;
            my_lp = __fsub_rn(bd, lsum);
        }
        if ((s & 63) == 63 || s == S - 1) {                                  // up to 64 samples per store, one per lane
            const int sl = (s & ~63) + lane;
            if (sl <= s) {
                idx_out[(size_t)row * S + sl] = my_idx;
                if (logp_out) logp_out[(size_t)row * S + sl] = my_lp;
            }
        }
    }
}
#undef VF_ROW_FOR

// ---------------------------------------------------------------- log-likelihood of a sampled view, one wave per (view, sample)
// ll[v][s] = the sum over the view's L tokens of logp[(v L + l) S + s] as ONE fp32 chain in token order (score_views_kernel's form: the
// lanes take 64 tokens at a time, their values are read back one by one and added in token order, the same on every lane)
__global__ __launch_bounds__(256) void sample_views_kernel(const float* __restrict__ logp, long long pairs, int L, int S, float* __restrict__ ll) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);     // p = v S + s
    if (p >= pairs) return;                                                 // a whole wave
    const long long v = p / S;
    const int s = (int)(p - v * S);
    float sum = 0.f;
    for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        const float lp = l < L ? logp[((size_t)v * L + l) * S + s] : 0.f;
        const int cnt = L - l0 < 64 ? L - l0 : 64;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            if (j < cnt) {
                const float xj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lp), j));
                sum = (l0 + j) ? __fadd_rn(sum, xj) : xj;
            }
        }
    }
    if (lane == 0) ll[p] = sum;
}

}  // namespace

extern "C" {

int vf_sample_rows_f32(const float* logits, int64_t rows, int N, int64_t ld, float temperature, int top_k, float top_p, uint32_t seed,
                       const int64_t* row_id, int S, int64_t* idx, float* logp, int32_t* kept, float* thr, void* stream) {
    if (!logits || !idx || rows < 0 || N < 1 || ld < N) return VF_ERR_BAD_ARG;
    if (!(temperature > 0.f) || !(temperature <= 3.402823466e38f)) return VF_ERR_BAD_ARG;      // <= 0, NaN, inf
    if (!(top_p > 0.f) || top_k < 0 || S < 1 || S > 65535) return VF_ERR_BAD_ARG;
    if (N > 65536 || rows > 0x7fffffffLL * 4) return VF_ERR_UNSUPPORTED;
    if (rows == 0) return VF_OK;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (N <= 1024)
        hipLaunchKernelGGL(sample_rows_kernel<true>, grid, block, 0, st, logits, (long long)rows, N, (long long)ld, temperature, top_k, top_p, seed,
                           reinterpret_cast<const long long*>(row_id), S, reinterpret_cast<long long*>(idx), logp, reinterpret_cast<int*>(kept), thr);
    else
        hipLaunchKernelGGL(sample_rows_kernel<false>, grid, block, 0, st, logits, (long long)rows, N, (long long)ld, temperature, top_k, top_p, seed,
                           reinterpret_cast<const long long*>(row_id), S, reinterpret_cast<long long*>(idx), logp, reinterpret_cast<int*>(kept), thr);
    return vf_last_status();
}

int vf_sample_views_f32(const float* logp, int64_t views, int L, int S, float* log_likelihood, void* stream) {
    if (!logp || !log_likelihood || views < 0 || L < 1 || S < 1 || S > 65535) return VF_ERR_BAD_ARG;
    if (views > 0x7fffffffLL * 4 / S) return VF_ERR_UNSUPPORTED;
    if (views == 0) return VF_OK;
    const long long pairs = (long long)views * S;
    hipLaunchKernelGGL(sample_views_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logp, pairs, L, S, log_likelihood);
    return vf_last_status();
}

}  // extern "C"
