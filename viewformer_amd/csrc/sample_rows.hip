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
// One wave per row.  N <= 1024: the row is read ONCE into registers (16 values per lane, lane-strided, coalesced; slots beyond N hold
// -inf, which nothing keeps) together with d_n = (z_n - max z) / T and e_n = e^d_n (exp_neg: lmhead_score.hip's, moved to vf_common.h), both
// computed once per row.  N > 1024: every pass re-reads the row (from cache) and recomputes d and e.  Everything after the read is
// wave-local: no LDS, no atomics.
//
// Thresholds are found on the ORDER-PRESERVING INTEGER IMAGE of the fp32 logits (sign bit flipped for positives, all bits for negatives:
// unsigned order = float order; dividing by T > 0 keeps the order, so the search runs on z and never sees a rounding): 32 steps from the
// top bit down, each step one masked count (top-k; ballots) or one masked mass (top-p; per-lane partial sums in slot order, then
// vf_wave_sum's butterfly).  Floating-point addition is monotone in each summand, so the mass in this FIXED order is monotone in the
// threshold and the search finds the largest threshold whose mass reaches the target — a value of the row.
//
// The key of the arg-max is d_n + g_n, not y_n + g_n: the same arg-max in exact arithmetic (a shift by max y), without |max y| in the
// rounding of the sum; logp = d_idx - log(sum_kept e) likewise.  -log u is formed as -log1p(-(1 - u)): 1 - u is exact in fp32 and the
// winners are the codes with u close to 1, where a plain fp32 log of u loses its relative accuracy.
//
// A row's outputs depend on its logits, the parameters, seed and row_id only: not on rows, on where the row sits, on ld, on S (sample s of
// any launch is sample s) or on the optional outputs requested.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

constexpr uint32_t SITE_SAMPLE = 0x5A0000u;
constexpr uint32_t IMG_NEG_INF = 0x007FFFFFu;             // image of -inf: below every finite value's

// unsigned image of a float with the floats' order (no NaN; -0 is canonicalised to +0 by the caller)
__device__ __forceinline__ uint32_t img_of(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float img_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// g = -log(-log u), u = ((w >> 9) + 0.5) 2^-23 in (0, 1): 1 - u is exact, -log u = -log1p(-(1 - u))
__device__ __forceinline__ float gumbel_of(uint32_t w) {
    const float u = __fmul_rn(__fadd_rn((float)(w >> 9), 0.5f), 1.1920928955078125e-7f);
    const float a = __fsub_rn(1.0f, u);
    return -logf(-log1pf(-a));
}

// Visits every element of the wave's row with (c, k, d, e) = (column, image of z, (z - max z) / T, e^d) in scope; all 64 lanes stay
// active (ballots and shuffles inside BODY are whole-wave).  REG: the 16 register slots; otherwise a pass over memory.
#define VF_ROW_FOR(...)                                                                                                       \
    if constexpr (REG) {                                                                                                        \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) {                                                                        \
            const int c = lane + 64 * j;                                                                                        \
            const uint32_t k = kimg[j];                                                                                         \
            const float d = dd[j], e = ee[j];                                                                                   \
            (void)c; (void)k; (void)d; (void)e;                                                                                 \
            __VA_ARGS__                                                                                                         \
        }                                                                                                                       \
    } else {                                                                                                                    \
        for (int c0 = 0; c0 < n; c0 += 64) {                                                                                    \
            const int c = c0 + lane;                                                                                            \
            const float zc = c < n ? __fadd_rn(xr[c], 0.0f) : -INFINITY;                                                        \
            const uint32_t k = img_of(zc);                                                                                      \
            const float d = __fdiv_rn(__fsub_rn(zc, zmax), T);                                                                  \
            const float e = k > IMG_NEG_INF ? exp_neg_clamped(d) : 0.0f;                                                        \
            (void)k; (void)d; (void)e;                                                                                          \
            __VA_ARGS__                                                                                                         \
        }                                                                                                                       \
    }

// e^d for d <= 0; arguments whose result is below the normal range anyway never reach exp_neg (d log2(e) would overflow for huge |d|)
__device__ __forceinline__ float exp_neg_clamped(float d) { return d >= -88.0f ? vf_exp_neg(d) : 0.0f; }

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

    // ---- the read (REG: the only one) and the row's maximum
    uint32_t kimg[16];
    float dd[16], ee[16];
    float zmax = -INFINITY;
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = lane + 64 * j;
            dd[j] = c < n ? __fadd_rn(xr[c], 0.0f) : -INFINITY;              // -0 -> +0: one image per value
            zmax = fmaxf(zmax, dd[j]);
        }
    } else {
        for (int c = lane; c < n; c += 64) zmax = fmaxf(zmax, xr[c]);
        zmax = __fadd_rn(zmax, 0.0f);
    }
    zmax = vf_wave_max(zmax);
    if (zmax == -INFINITY) {                                                // no finite logit: no distribution (uniform over the wave)
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
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float zc = dd[j];
            kimg[j] = img_of(zc);
            dd[j] = __fdiv_rn(__fsub_rn(zc, zmax), T);
            ee[j] = kimg[j] > IMG_NEG_INF ? exp_neg_clamped(dd[j]) : 0.0f;
        }
    }
    const uint32_t kmax = img_of(zmax);

    // ---- top-k: the image of the k-th largest value, or of the smallest finite one where top-k does not apply
    int nfinite = 0;
    uint32_t kmin = 0xFFFFFFFFu;
    VF_ROW_FOR(nfinite += __popcll(__ballot(k > IMG_NEG_INF)); kmin = k > IMG_NEG_INF && k < kmin ? k : kmin;)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)kmin, o, 64);
        kmin = ok < kmin ? ok : kmin;
    }
    uint32_t t = kmin;
    if (top_k > 0 && top_k < nfinite) {
        t = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            int cnt = 0;
            VF_ROW_FOR(cnt += __popcll(__ballot(k >= cand));)
            t = cnt >= top_k ? cand : t;
        }
    }

    // ---- top-p: the largest threshold whose mass reaches top_p x the mass top-k left
    float mass;
    {
        float part = 0.f;
        VF_ROW_FOR(part = __fadd_rn(part, k >= t ? e : 0.0f);)
        mass = vf_wave_sum(part);
    }
    if (top_p < 1.0f) {
        const float target = __fmul_rn(top_p, mass);
        const uint32_t tk = t;
        uint32_t tp = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = tp | (1u << bit);
            float part = 0.f;
            VF_ROW_FOR(part = __fadd_rn(part, (k >= cand && k >= tk) ? e : 0.0f);)
            tp = vf_wave_sum(part) >= target ? cand : tp;
        }
        tp = tp > kmax ? kmax : tp;                                          // the maximum is always kept
        t = tp > tk ? tp : tk;
        float part = 0.f;
        VF_ROW_FOR(part = __fadd_rn(part, k >= t ? e : 0.0f);)
        mass = vf_wave_sum(part);
    }
    const float lsum = logf(mass);                                           // mass >= 1: the maximum's e is exactly 1
    if (kept_out || thr_out) {
        int cnt = 0;
        VF_ROW_FOR(cnt += __popcll(__ballot(k >= t));)
        if (lane == 0) {
            if (kept_out) kept_out[row] = cnt;
            if (thr_out) thr_out[row] = __fdiv_rn(img_inv(t), T);
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
