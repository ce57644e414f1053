// The kept set of a row of logits under temperature, top-k and top-p — steps (1)-(3) of vf_sample_rows_f32 (include/vf_hip.h, DESIGN.md
// §6.15) — for one wave per row.  Shared by sample_rows.hip (which draws from the set) and mix_rows.hip (which averages the codebook over
// it), so that both report the same set, threshold and mass bit for bit.
//
// N <= 1024 (REG): the row is read ONCE into registers (16 values per lane, lane-strided, coalesced; slots beyond N hold -inf, which nothing
// keeps) together with d_n = (z_n - max z) / T and e_n = e^d_n, both computed once per row.  N > 1024: every pass re-reads the row (from
// cache) and recomputes d and e.  Everything after the read is wave-local: no LDS, no atomics.
//
// Thresholds are found on the ORDER-PRESERVING INTEGER IMAGE of the fp32 logits (sign bit flipped for positives, all bits for negatives:
// unsigned order = float order; dividing by T > 0 keeps the order, so the search runs on z and never sees a rounding): 32 steps from the
// top bit down, each step one masked count (top-k; ballots) or one masked mass (top-p; per-lane partial sums in slot order, then
// vf_wave_sum's butterfly).  Floating-point addition is monotone in each summand, so the mass in this FIXED order is monotone in the
// threshold and the search finds the largest threshold whose mass reaches the target — a value of the row.
#pragma once
#include "vf_common.h"

constexpr uint32_t VF_IMG_NEG_INF = 0x007FFFFFu;             // image of -inf: below every finite value's

// unsigned image of a float with the floats' order (no NaN; -0 is canonicalised to +0 by the caller)
__device__ __forceinline__ uint32_t vf_img_of(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float vf_img_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// e^d for d <= 0; arguments whose result is below the normal range anyway never reach exp_neg (d log2(e) would overflow for huge |d|)
__device__ __forceinline__ float vf_exp_neg_clamped(float d) { return d >= -88.0f ? vf_exp_neg(d) : 0.0f; }

// Visits every element of the wave's row with (c, k, d, e) = (column, image of z, (z - max z) / T, e^d) in scope; all 64 lanes stay
// active (ballots and shuffles inside BODY are whole-wave).  REG: the 16 register slots; otherwise a pass over memory.  Expects REG, lane,
// n, xr, zmax, T and (REG) kimg / dd / ee in scope: vf_row_filter's, and its callers' under the same names.
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
            const uint32_t k = vf_img_of(zc);                                                                                   \
            const float d = __fdiv_rn(__fsub_rn(zc, zmax), T);                                                                  \
            const float e = k > VF_IMG_NEG_INF ? vf_exp_neg_clamped(d) : 0.0f;                                                  \
            (void)k; (void)d; (void)e;                                                                                          \
            __VA_ARGS__                                                                                                         \
        }                                                                                                                       \
    }

// The whole wave calls it on its row xr[0..n).  -> false: the row has no finite logit (nothing else is set).  Otherwise zmax = max z,
// t = the image of the smallest kept logit (the kept set is {c : k_c >= t}), mass = the sum of e over the kept set in the fixed order above
// (>= 1: the maximum's e is exactly 1), and with REG the row's kimg / dd / ee in the caller's registers.
template <bool REG>
__device__ __forceinline__ bool vf_row_filter(const float* __restrict__ xr, int n, int lane, float T, int top_k, float top_p,
                                              uint32_t (&kimg)[16], float (&dd)[16], float (&ee)[16], float& zmax, uint32_t& t, float& mass) {
    // ---- the read (REG: the only one) and the row's maximum
    zmax = -INFINITY;
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
    if (zmax == -INFINITY) return false;                                    // no finite logit: no distribution (uniform over the wave)
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float zc = dd[j];
            kimg[j] = vf_img_of(zc);
            dd[j] = __fdiv_rn(__fsub_rn(zc, zmax), T);
            ee[j] = kimg[j] > VF_IMG_NEG_INF ? vf_exp_neg_clamped(dd[j]) : 0.0f;
        }
    }
    const uint32_t kmax = vf_img_of(zmax);

    // ---- top-k: the image of the k-th largest value, or of the smallest finite one where top-k does not apply
    int nfinite = 0;
    uint32_t kmin = 0xFFFFFFFFu;
    VF_ROW_FOR(nfinite += __popcll(__ballot(k > VF_IMG_NEG_INF)); kmin = k > VF_IMG_NEG_INF && k < kmin ? k : kmin;)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)kmin, o, 64);
        kmin = ok < kmin ? ok : kmin;
    }
    t = kmin;
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
    return true;
}
