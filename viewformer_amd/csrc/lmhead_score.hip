// Tied LM head with the soft-max statistics fused into its epilogue, bf16 arm, gfx950 — and the same statistics from materialised logits.
//
// "How well does this photo fit this camera?" is the token log-likelihood of the photo's codes under the MASK view at that pose:
// log p[m][target[m]] = z[m][target[m]] - lse[m], z[m][n] = sum_k bf16(h[m][k]) * bf16(wte[n][k]).  Through the logits that is a [M][N] fp32
// store (4 KiB per row at 1024 codes), a log_softmax that reads them and writes as much again, and a gather; five numbers per row survive.
// vf_lmhead_score_bf16 is csrc/lmhead_argmax.hip's walk (one workgroup = 32 rows in registers x all codes, 4 waves x a quarter of the codes
// in 32-wide tiles, the packed wte streamed once) whose epilogue carries, beside the running arg-max, the online soft-max sums — the
// logits are never stored.  Same operands, same k order and one fp32 accumulation chain per (row, code) as vf_gemm_bf16 and
// vf_lmhead_argmax_bf16 on the same packing: idx / max_logit are the arg-max kernel's bits, target_logit is the bit pattern the GEMM stores.
//
// Per row:   max, idx (first maximum);   s = sum_n e^(z_n - max);   t = sum_n (z_n - max) e^(z_n - max)
//            lse = max + log s;   entropy = lse - sum_n p_n z_n = log s - t / s   (p_n = e^(z_n - lse))
// Online form per lane (its codes ascending), then merges in a fixed order (xor butterfly 16, 8, 4, 2, 1 over the 32 code lanes of a
// half-wave, then waves 0..3 through LDS).  When the reference maximum moves by d <= 0:  s <- s e^d,  t <- (t + d s) e^d.
// Everything is computed whatever outputs were asked for, rows beyond M repeat row M - 1 and are not stored, no atomics: a row's outputs
// do not depend on M, on where the row sits or on the set of outputs requested.
//
// vf_logits_score_f32: the same five numbers from fp32 logits [rows][ld] (the fp32-equivalent arms, and shapes the fused kernel refuses):
// one wave per row, pass 1 max / first index, pass 2 the two sums from lane-strided partials and vf_wave_sum's butterfly.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BN = 128;                   // the bf16 weight packing's chunk / n-block (csrc/gemm_bf16.hip)

// (max, first index, s, t) of one set of codes absorbs another's: the side with the smaller maximum is rescaled by e^-(difference).
// Symmetric (both partners of a butterfly step end with the same bits): the sums are commutative, equal maxima rescale by exactly 1.
__device__ __forceinline__ void merge(float& m, int& i, float& s, float& t, float om, int oi, float os, float ot) {
    const float d = -fabsf(__fsub_rn(m, om));
    const float e = vf_exp_neg(d);
    const bool other_wins = om > m;
    const float ls = other_wins ? s : os, lt = other_wins ? t : ot;           // the lower side, to be rescaled
    const float hs = other_wins ? os : s, ht = other_wins ? ot : t;
    s = __fadd_rn(hs, __fmul_rn(ls, e));
    t = __fadd_rn(ht, __fmul_rn(__fadd_rn(lt, __fmul_rn(d, ls)), e));
    if (other_wins || (om == m && oi < i)) { m = om; i = oi; }
}

template <int KSTEPS>
__global__ __launch_bounds__(256, 1) void lmhead_score_kernel(const void* __restrict__ hrows, int h16, long long ldh,
                                                              const unsigned char* __restrict__ Wp, long long M, int N,
                                                              const int* __restrict__ target, long long* __restrict__ idx_out,
                                                              float* __restrict__ max_out, float* __restrict__ lse_out,
                                                              float* __restrict__ tgt_out, float* __restrict__ ent_out) {
    __shared__ float red_m[4][32], red_s[4][32], red_t[4][32];
    __shared__ int red_i[4][32];
    __shared__ int tgt_n[32];
    __shared__ float tgt_z[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const long long m0 = (long long)blockIdx.x * 32;
    long long row = m0 + l31;
    row = row < M ? row : M - 1;
    if (tid < 32) {
        tgt_n[tid] = target ? target[row] : -1;          // compared with code numbers only: a target outside [0, N) matches none
        tgt_z[tid] = -INFINITY;
    }

    bf16x8 a[KSTEPS];
    if (h16) {
        const __bf16* src = reinterpret_cast<const __bf16*>(hrows) + (size_t)row * ldh + half * 8;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) a[ks] = *reinterpret_cast<const bf16x8*>(src + ks * 16);
    } else {
        const float* src = reinterpret_cast<const float*>(hrows) + (size_t)row * ldh + half * 8;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(src + ks * 16);
            const f32x4 t1 = *reinterpret_cast<const f32x4*>(src + ks * 16 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[ks][e] = (__bf16)t0[e]; a[ks][4 + e] = (__bf16)t1[e]; }
        }
    }
    __syncthreads();                                     // tgt_n / tgt_z are set before any wave's first tile

    const int nb = N / BN;
    const int tiles_per_wave = N / 4 / 32;
    // per accumulator row r (row (r&3) + 8 (r>>2) + 4 half of the tile, code l31 of each tile): the online triple and the first arg-max
    float best[16], sum[16], tsum[16];
    int besti[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { best[r] = -INFINITY; besti[r] = 0; sum[r] = 0.f; tsum[r] = 0.f; }
    for (int nt = 0; nt < tiles_per_wave; ++nt) {
        const int n0 = wave * (N / 4) + nt * 32;
        const int nblk = n0 / BN, nl = (n0 % BN) + l31;
        // fragment (chunk, ks) of column n: ((((chunk*nb + nblk)*4 + ks)*2 + half)*128 + nl) * 16 bytes
        const unsigned char* wsrc = Wp + ((size_t)nblk * 8 + half) * (BN * 16) + (size_t)nl * 16;
        const size_t chunk_stride = (size_t)nb * 8 * BN * 16;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(wsrc + (size_t)(ks >> 2) * chunk_stride + (size_t)(ks & 3) * (2 * BN * 16));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks], b, acc, 0, 0, 0);
        }
        const int n = n0 + l31;
        if (nt == 0) {                                   // the lane's first code: the triple of one element, (z, 1, 0)
#pragma unroll
            for (int r = 0; r < 16; ++r) { best[r] = acc[r]; besti[r] = n; sum[r] = 1.f; tsum[r] = 0.f; }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float z = acc[r];
                const bool up = z > best[r];                                    // strict: the first maximum of this lane's (ascending) codes
                const float d = -fabsf(__fsub_rn(z, best[r]));
                const float e = vf_exp_neg(d);
                const float s_up = __fadd_rn(__fmul_rn(sum[r], e), 1.f);        // the maximum moves by d: rescale, then the new code's (1, 0)
                const float t_up = __fmul_rn(__fadd_rn(tsum[r], __fmul_rn(d, sum[r])), e);
                const float s_dn = __fadd_rn(sum[r], e);
                const float t_dn = __fadd_rn(tsum[r], __fmul_rn(d, e));
                sum[r] = up ? s_up : s_dn;
                tsum[r] = up ? t_up : t_dn;
                best[r] = up ? z : best[r];
                besti[r] = up ? n : besti[r];
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (tgt_n[(r & 3) + 8 * (r >> 2) + 4 * half] == n) tgt_z[(r & 3) + 8 * (r >> 2) + 4 * half] = acc[r];   // one lane of the workgroup per row
    }
    // reduce over the 32 lanes (codes) of the half-wave
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = best[r], s = sum[r], t = tsum[r];
        int i = besti[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64), os = __shfl_xor(s, o, 64), ot = __shfl_xor(t, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            merge(v, i, s, t, ov, oi, os, ot);
        }
        if (l31 == 0) {
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * half;
            red_m[wave][rl] = v;
            red_i[wave][rl] = i;
            red_s[wave][rl] = s;
            red_t[wave][rl] = t;
        }
    }
    __syncthreads();
    if (tid < 32) {
        float v = red_m[0][tid], s = red_s[0][tid], t = red_t[0][tid];
        int i = red_i[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) merge(v, i, s, t, red_m[w][tid], red_i[w][tid], red_s[w][tid], red_t[w][tid]);
        if (m0 + tid < M) {
            const float ls = logf(s);
            if (idx_out) idx_out[m0 + tid] = (long long)i;
            if (max_out) max_out[m0 + tid] = v;
            if (lse_out) lse_out[m0 + tid] = __fadd_rn(v, ls);
            if (tgt_out) tgt_out[m0 + tid] = tgt_z[tid];
            if (ent_out) ent_out[m0 + tid] = __fsub_rn(ls, t / s);
        }
    }
}

// ---------------------------------------------------------------- the same statistics of fp32 logits, one wave per row
__global__ __launch_bounds__(256) void logits_score_kernel(const float* __restrict__ x, long long rows, int n, long long ld,
                                                           const int* __restrict__ target, long long* __restrict__ idx_out,
                                                           float* __restrict__ max_out, float* __restrict__ lse_out,
                                                           float* __restrict__ tgt_out, float* __restrict__ ent_out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * ld;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < n; c += 64) {
        const float v = xr[c];
        if (v > bv || bi == 0x7fffffff) { bv = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    float s = 0.f, t = 0.f;
    for (int c = lane; c < n; c += 64) {
        const float d = __fsub_rn(xr[c], bv);
        const float e = expf(d);
        s = __fadd_rn(s, e);
        t = __fadd_rn(t, e > 0.f ? __fmul_rn(d, e) : 0.f);               // p = 0 contributes 0 to sum p z, also at z = -inf
    }
    s = vf_wave_sum(s);
    t = vf_wave_sum(t);
    if (lane == 0) {
        const float ls = logf(s);
        const bool empty = bv == -INFINITY;                                // every logit -inf: lse = -inf (as logsumexp), no distribution
        if (idx_out) idx_out[row] = bi == 0x7fffffff ? 0 : bi;
        if (max_out) max_out[row] = bv;
        if (lse_out) lse_out[row] = empty ? -INFINITY : __fadd_rn(bv, ls);
        if (ent_out) ent_out[row] = empty ? __builtin_nanf("") : __fsub_rn(ls, t / s);
        if (tgt_out) {
            const int tg = target[row];
            tgt_out[row] = (tg >= 0 && tg < n) ? xr[tg] : -INFINITY;
        }
    }
}

// ---------------------------------------------------------------- per-view summary of the row statistics, one wave per view
// lanes take a view's rows 64 at a time (coalesced); the log-likelihood is ONE fp32 chain in token order: the lanes' values are read
// back one by one (v_readlane with a constant lane) and added in row order, the same on every lane
__global__ __launch_bounds__(256) void score_views_kernel(const float* __restrict__ tgt, const float* __restrict__ lse, const float* __restrict__ mx,
                                                          const long long* __restrict__ idx, const int* __restrict__ target, long long views,
                                                          int L, float* __restrict__ tlp, float* __restrict__ conf, float* __restrict__ ll,
                                                          float* __restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const long long v = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= views) return;                                                 // a whole wave
    float sum = 0.f;
    int hits = 0;
    for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        float lp = 0.f;
        bool hit = false;
        if (l < L) {
            const size_t r = (size_t)v * L + l;
            lp = __fsub_rn(tgt[r], lse[r]);
            tlp[r] = lp;
            conf[r] = __fsub_rn(mx[r], lse[r]);
            hit = idx[r] == (long long)target[r];
        }
        hits += __popcll(__ballot(hit));
        const int n = L - l0 < 64 ? L - l0 : 64;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            if (j < n) {
                const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lp), j));
                sum = (l0 + j) ? __fadd_rn(sum, x) : x;
            }
        }
    }
    if (lane == 0) {
        ll[v] = sum;
        acc[v] = (float)hits / (float)L;
    }
}

}  // namespace

extern "C" {

int vf_lmhead_score_bf16(const void* h, int h_bf16, int64_t ldh, const void* w_packed, int64_t M, int K, int N, const int32_t* target,
                         int64_t* idx, float* max_logit, float* lse, float* target_logit, float* entropy, void* stream) {
    if (!h || !w_packed || M < 0 || K <= 0 || N <= 0 || ldh < K) return VF_ERR_BAD_ARG;
    if (!idx && !max_logit && !lse && !target_logit && !entropy) return VF_ERR_BAD_ARG;
    if (target_logit && !target) return VF_ERR_BAD_ARG;
    if (N % BN != 0 || (K != 768 && K != 128) || (h_bf16 ? (ldh & 7) : (ldh & 3)) || M > 0x7fffffffLL * 32) return VF_ERR_UNSUPPORTED;
    if (M == 0) return VF_OK;
    const unsigned grid = (unsigned)((M + 31) / 32);
    hipStream_t s = (hipStream_t)stream;
    const unsigned char* wp = reinterpret_cast<const unsigned char*>(w_packed);
    if (K == 768)
        hipLaunchKernelGGL(lmhead_score_kernel<48>, dim3(grid), dim3(256), 0, s, h, h_bf16, (long long)ldh, wp, (long long)M, N,
                           reinterpret_cast<const int*>(target), reinterpret_cast<long long*>(idx), max_logit, lse, target_logit, entropy);
    else
        hipLaunchKernelGGL(lmhead_score_kernel<8>, dim3(grid), dim3(256), 0, s, h, h_bf16, (long long)ldh, wp, (long long)M, N,
                           reinterpret_cast<const int*>(target), reinterpret_cast<long long*>(idx), max_logit, lse, target_logit, entropy);
    return vf_last_status();
}

int vf_logits_score_f32(const float* logits, int64_t rows, int N, int64_t ld, const int32_t* target, int64_t* idx, float* max_logit,
                        float* lse, float* target_logit, float* entropy, void* stream) {
    if (!logits || rows < 0 || N <= 0 || ld < N) return VF_ERR_BAD_ARG;
    if (!idx && !max_logit && !lse && !target_logit && !entropy) return VF_ERR_BAD_ARG;
    if (target_logit && !target) return VF_ERR_BAD_ARG;
    if (rows > 0x7fffffffLL * 4) return VF_ERR_UNSUPPORTED;
    if (rows == 0) return VF_OK;
    hipLaunchKernelGGL(logits_score_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, (long long)rows, N,
                       (long long)ld, reinterpret_cast<const int*>(target), reinterpret_cast<long long*>(idx), max_logit, lse, target_logit,
                       entropy);
    return vf_last_status();
}

int vf_score_views_f32(const float* target_logit, const float* lse, const float* max_logit, const int64_t* idx, const int32_t* target,
                       int64_t views, int L, float* token_log_prob, float* confidence, float* log_likelihood, float* accuracy, void* stream) {
    if (!target_logit || !lse || !max_logit || !idx || !target || !token_log_prob || !confidence || !log_likelihood || !accuracy || views < 0 ||
        L <= 0)
        return VF_ERR_BAD_ARG;
    if (views > 0x7fffffffLL * 4) return VF_ERR_UNSUPPORTED;
    if (views == 0) return VF_OK;
    hipLaunchKernelGGL(score_views_kernel, dim3((unsigned)((views + 3) / 4)), dim3(256), 0, (hipStream_t)stream, target_logit, lse, max_logit,
                       reinterpret_cast<const long long*>(idx), reinterpret_cast<const int*>(target), (long long)views, L, token_log_prob, confidence,
                       log_likelihood, accuracy);
    return vf_last_status();
}

}  // extern "C"
