// Backward of the prefix-cache attention (attention_prefix.hip) over the QUERY views only, exact-f32 MFMA, gfx950: the gradient of a loss
// with respect to a query view's own q / k / v, given the gradient of its attention output.  The cached context does not depend on the
// query camera, so nothing flows into the cache: per (scene, view, head) the kernel needs
//     dQ = dS . [Kp; K]          (all keys the view walks: its ctx_len prefix tiles, then its own tile)
//     dK = dS_own^T . Q,  dV = P_own^T . dO          (the view's own 64 keys only)
// with  S = Q K^T (un-scaled, as the forward),  P = exp(S - lse),  dP = dO . V^T,  dS = P * (dP - D),  D = rowsum(dO * O).
// O and lse are RECOMPUTED here in fp32 from the operands as stored (the forward's output is bf16 on one arm and carries no lse).
//
// One kernel for both arms: operands are widened to fp32 on load (in_bf16: q / k / v / kp / vp are bf16 storage), every product runs on
// v_mfma_f32_32x32x2_f32 with the operand / accumulator layouts of attention_bwd_f32.hip (the "owner" of a product sits in the MFMA
// column = lane, so P / dS are born in the B-operand layout of the accumulation that follows; its A operand is a transposed LDS tile).
//
// Work layout: one workgroup of 128 threads per (scene, view, head); wave w owns the queries 32 w ... 32 w + 31 (passes 1 and 2) and the
// keys 32 w ... 32 w + 31 of the own tile (dK / dV).  No reduction crosses waves or workgroups; no atomics; tiles are walked in a fixed
// order (prefix ascending, own tile last), each 64-key tile as two 32-key steps:
//   pass 1  per step: S^T = K.Q^T, running max / sum (rescale per step), O^T += V^T.P^T      -> lse = m + log l,  D = (dO . O~) / l
//   pass 2  per step: S^T, dP^T = V.dO^T, dS^T = P (dP - D), dQ^T += K^T.dS^T                -> dQ
//   own     lane = key: S = Q.K^T, dP = dO.V^T per 32-query half, dV^T += dO^T.P, dK^T += Q^T.dS   -> dK, dV
// A view's arithmetic depends on its own rows and on the first ctx_len tiles of its scene's cache, nothing else: its result is bit-identical
// whatever N, its position, the other views' lengths and the cache's capacity, and no cache row at or beyond its length is read.
// Output: dqkv rows in the c_attn column order (V, Q, K) — dV in [0, d), dQ in [d, 2d), dK in [2d, 3d), d = 64 H — every element of
// every row written exactly once, nothing else.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int DH = 64;
constexpr int LV = 64;      // tokens per view = keys per tile
constexpr int LD = 68;      // LDS row stride in floats: attention_bwd_f32.hip's padding (rows stay 16-byte aligned for ds_read_b128)
constexpr int NT = 128;     // threads per workgroup
constexpr float LOG2E = 1.4426950408889634f;
constexpr size_t SMEM = (size_t)(4 * LV * LD + 2 * LV) * sizeof(float);

struct pbwd_args {
    const void* q; const void* k; const void* v;      // query views' thirds of the fused c_attn output, rows [B*N*L]
    const void* kp; const void* vp;                   // prefix K / V, rows [C*L] per scene, scenes pstride elements apart
    const float* dout;
    float* dqkv;
    const int* ctx_len;                               // [B*N] or nullptr (all C)
    int C, N, H;
    int ldq, ldk, ldv, ldkp, ldvp, lddo, lddqkv;
    long long pstride;
    int in16;
};

__device__ __forceinline__ f32x4 load4(const void* base, size_t off, int in16) {
    if (in16) {
        const bf16x4 t = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(base) + off);
        return f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
    }
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + off);
}

// 64 rows x 64 features from global (row r at element off0 + r ld) into LDS: row-major into R and / or transposed into T
__device__ __forceinline__ void stage64(const void* base, size_t off0, int ld, int in16, float* R, float* T) {
    const int s_col4 = threadIdx.x & 15, s_row0 = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = s_row0 + 8 * i;
        const f32x4 a = load4(base, off0 + (size_t)row * ld + s_col4 * 4, in16);
        if (R) *reinterpret_cast<f32x4*>(R + row * LD + s_col4 * 4) = a;
        if (T) {
#pragma unroll
            for (int e = 0; e < 4; ++e) T[(s_col4 * 4 + e) * LD + row] = a[e];
        }
    }
}

// one row's 64 features as the B operand of the 32x32x2 products: reg[4 g + e] = row[8 g + 4 half + e]
__device__ __forceinline__ void load_row(const void* base, size_t off, int in16, int half, float* reg) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const f32x4 t = load4(base, off + 8 * g + 4 * half, in16);
#pragma unroll
        for (int e = 0; e < 4; ++e) reg[g * 4 + e] = t[e];
    }
}

__device__ __forceinline__ void store_acc(float* row, const f32x16 (&acc)[2]) {      // row already at + 4 half
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = acc[d][4 * j + e];
            *reinterpret_cast<f32x4*>(row + d * 32 + 8 * j) = o;
        }
}

__global__ __launch_bounds__(NT) void attn_prefix_bwd_kernel(const pbwd_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem_pb[];
    float* A0 = smem_pb;                // K rows          | own phase: Q rows
    float* A1 = A0 + LV * LD;           // V rows          | own phase: dO rows
    float* A2 = A1 + LV * LD;           // V^T (pass 1), K^T (pass 2) | own phase: Q^T
    float* A3 = A2 + LV * LD;           //                 | own phase: dO^T
    float* Ls = A3 + LV * LD;           // [64] lse
    float* Ds = Ls + LV;                // [64] D

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int h = blockIdx.x;
    const size_t b = blockIdx.y;
    const int n = blockIdx.z;
    const int in16 = a.in16;
    const size_t view = b * (size_t)a.N + (size_t)n;
    const size_t row0 = view * LV;                               // the view's first row
    const int len = a.ctx_len ? min(max(a.ctx_len[view], 0), a.C) : a.C;
    const int d = a.H * DH;

    const size_t qrow = row0 + wave * 32 + l31;
    float qreg[32], doreg[32];
    load_row(a.q, qrow * a.ldq + h * DH, in16, half, qreg);
    load_row(a.dout, qrow * a.lddo + h * DH, 0, half, doreg);

    auto koff = [&](int s, const void*& base, int& ld) -> size_t {       // K of tile s (s == len: the own tile)
        if (s < len) { base = a.kp; ld = a.ldkp; return b * (size_t)a.pstride + (size_t)s * LV * a.ldkp + h * DH; }
        base = a.k; ld = a.ldk; return row0 * a.ldk + h * DH;
    };
    auto voff = [&](int s, const void*& base, int& ld) -> size_t {
        if (s < len) { base = a.vp; ld = a.ldvp; return b * (size_t)a.pstride + (size_t)s * LV * a.ldvp + h * DH; }
        base = a.v; ld = a.ldv; return row0 * a.ldv + h * DH;
    };

    // ---------------------------------------------------------------------------------------------------- pass 1: lse and D
    float lse_q, D_q;
    {
        f32x16 ot[2];
#pragma unroll
        for (int dd = 0; dd < 2; ++dd)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dd][r] = 0.f;
        float m_run = -INFINITY, l_run = 0.f;
        for (int s = 0; s <= len; ++s) {
            const void *kb, *vb;
            int ldk_, ldv_;
            const size_t k0 = koff(s, kb, ldk_), v0 = voff(s, vb, ldv_);
            __syncthreads();                                         // previous tile fully consumed
            stage64(kb, k0, ldk_, in16, A0, nullptr);
            stage64(vb, v0, ldv_, in16, nullptr, A2);
            __syncthreads();
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                f32x16 st;
#pragma unroll
                for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const f32x4 kk = *reinterpret_cast<const f32x4*>(A0 + (t2 * 32 + l31) * LD + 8 * g + 4 * half);
#pragma unroll
                    for (int e = 0; e < 4; ++e) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kk[e], qreg[g * 4 + e], st, 0, 0, 0);      // S^T = K.Q^T
                }
                float mx = st[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float m_new = fmaxf(m_run, mx);
                const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);      // 0 on the first step (m_run = -inf)
                float psum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f((st[r] - m_new) * LOG2E);
                    st[r] = p;
                    psum += p;
                }
                l_run = l_run * alpha + psum;
                m_run = m_new;
#pragma unroll
                for (int dd = 0; dd < 2; ++dd)
#pragma unroll
                    for (int r = 0; r < 16; ++r) ot[dd][r] *= alpha;
                // O^T[feature][query] += V^T[feature][key] . P^T[key][query]
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4 vv[2];
#pragma unroll
                    for (int dd = 0; dd < 2; ++dd)
                        vv[dd] = *reinterpret_cast<const f32x4*>(A2 + (dd * 32 + l31) * LD + t2 * 32 + 8 * j + 4 * half);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int dd = 0; dd < 2; ++dd)
                            ot[dd] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[dd][e], st[4 * j + e], ot[dd], 0, 0, 0);
                }
            }
        }
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        // accumulator register 4 j + e of half-tile dd = feature 32 dd + 8 j + 4 half + e = doreg[4 (4 dd + j) + e]
        float dsum = 0.f;
#pragma unroll
        for (int dd = 0; dd < 2; ++dd)
#pragma unroll
            for (int r = 0; r < 16; ++r) dsum = __builtin_fmaf(ot[dd][r], doreg[16 * dd + r], dsum);
        dsum += __shfl_xor(dsum, 32, 64);
        D_q = dsum / l_tot;
        lse_q = m_run + logf(l_tot);
    }

    // ---------------------------------------------------------------------------------------------------- pass 2: dQ
    {
        f32x16 ot[2];
#pragma unroll
        for (int dd = 0; dd < 2; ++dd)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dd][r] = 0.f;
        for (int s = 0; s <= len; ++s) {
            const void *kb, *vb;
            int ldk_, ldv_;
            const size_t k0 = koff(s, kb, ldk_), v0 = voff(s, vb, ldv_);
            __syncthreads();
            stage64(kb, k0, ldk_, in16, A0, A2);
            stage64(vb, v0, ldv_, in16, A1, nullptr);
            __syncthreads();
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                f32x16 st, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const f32x4 kk = *reinterpret_cast<const f32x4*>(A0 + (t2 * 32 + l31) * LD + 8 * g + 4 * half);
                    const f32x4 vv = *reinterpret_cast<const f32x4*>(A1 + (t2 * 32 + l31) * LD + 8 * g + 4 * half);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kk[e], qreg[g * 4 + e], st, 0, 0, 0);      // S^T = K.Q^T
                        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[e], doreg[g * 4 + e], dp, 0, 0, 0);     // dP^T = V.dO^T
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f((st[r] - lse_q) * LOG2E);
                    st[r] = p * (dp[r] - D_q);                                   // dS^T
                }
                // dQ^T[feature][query] += K^T[feature][key] . dS^T[key][query]
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4 kk[2];
#pragma unroll
                    for (int dd = 0; dd < 2; ++dd)
                        kk[dd] = *reinterpret_cast<const f32x4*>(A2 + (dd * 32 + l31) * LD + t2 * 32 + 8 * j + 4 * half);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int dd = 0; dd < 2; ++dd)
                            ot[dd] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk[dd][e], st[4 * j + e], ot[dd], 0, 0, 0);
                }
            }
        }
        store_acc(a.dqkv + qrow * (size_t)a.lddqkv + d + h * DH + 4 * half, ot);
    }

    // ---------------------------------------------------------------------------------------------------- own tile: dK, dV (lane = key)
    __syncthreads();
    stage64(a.q, row0 * a.ldq + h * DH, a.ldq, in16, A0, A2);
    stage64(a.dout, row0 * a.lddo + h * DH, a.lddo, 0, A1, A3);
    if (half == 0) { Ls[wave * 32 + l31] = lse_q; Ds[wave * 32 + l31] = D_q; }
    __syncthreads();
    {
        float kreg[32], vreg[32];
        load_row(a.k, qrow * a.ldk + h * DH, in16, half, kreg);      // (qrow: the lane's row of the view, now as a key)
        load_row(a.v, qrow * a.ldv + h * DH, in16, half, vreg);
        f32x16 okt[2], ovt[2];
#pragma unroll
        for (int dd = 0; dd < 2; ++dd)
#pragma unroll
            for (int r = 0; r < 16; ++r) { okt[dd][r] = 0.f; ovt[dd][r] = 0.f; }
#pragma unroll 1
        for (int t2 = 0; t2 < 2; ++t2) {                             // the two 32-query halves, ascending
            f32x16 st, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 qq = *reinterpret_cast<const f32x4*>(A0 + (t2 * 32 + l31) * LD + 8 * g + 4 * half);
                const f32x4 oo = *reinterpret_cast<const f32x4*>(A1 + (t2 * 32 + l31) * LD + 8 * g + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    st = __builtin_amdgcn_mfma_f32_32x32x2f32(qq[e], kreg[g * 4 + e], st, 0, 0, 0);          // S = Q.K^T
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(oo[e], vreg[g * 4 + e], dp, 0, 0, 0);          // dP = dO.V^T
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = t2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;      // query row inside the view
                const float p = __builtin_amdgcn_exp2f((st[r] - Ls[ql]) * LOG2E);
                st[r] = p;
                dp[r] = p * (dp[r] - Ds[ql]);                                    // dS
            }
            // dV^T[feature][key] += dO^T[feature][query] . P[query][key];  dK^T[feature][key] += Q^T[feature][query] . dS[query][key]
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 oo[2], qq[2];
#pragma unroll
                for (int dd = 0; dd < 2; ++dd) {
                    oo[dd] = *reinterpret_cast<const f32x4*>(A3 + (dd * 32 + l31) * LD + t2 * 32 + 8 * j + 4 * half);
                    qq[dd] = *reinterpret_cast<const f32x4*>(A2 + (dd * 32 + l31) * LD + t2 * 32 + 8 * j + 4 * half);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int dd = 0; dd < 2; ++dd) {
                        ovt[dd] = __builtin_amdgcn_mfma_f32_32x32x2f32(oo[dd][e], st[4 * j + e], ovt[dd], 0, 0, 0);
                        okt[dd] = __builtin_amdgcn_mfma_f32_32x32x2f32(qq[dd][e], dp[4 * j + e], okt[dd], 0, 0, 0);
                    }
            }
        }
        float* orow = a.dqkv + qrow * (size_t)a.lddqkv + h * DH + 4 * half;
        store_acc(orow, ovt);                   // dV: columns [0, d)
        store_acc(orow + 2 * d, okt);           // dK: columns [2d, 3d)
    }
}

}  // namespace

extern "C" int vf_attn_prefix_bwd_f32(const void* q, const void* k, const void* v, const void* kp, const void* vp, int in_bf16,
                                      const float* dout, float* dqkv, int B, int H, int C, int N, int L, int dh, int ldq, int ldk, int ldv,
                                      int ldkp, int ldvp, int64_t prefix_stride, int lddo, int lddqkv, const int32_t* ctx_len, void* stream) {
    if (B < 0 || N < 0 || H <= 0 || C < 0) return VF_ERR_BAD_ARG;
    if (!q || !k || !v || !kp || !vp || !dout || !dqkv) return VF_ERR_BAD_ARG;
    if (L != LV || dh != DH || C < 1) return VF_ERR_UNSUPPORTED;
    if (H > 65535) return VF_ERR_UNSUPPORTED;                        // grid dimension x (and 3 * 64 * H stays far inside int)
    const int w = H * DH;
    if (ldq < w || ldk < w || ldv < w || ldkp < w || ldvp < w || lddo < w || lddqkv < 3 * w) return VF_ERR_BAD_ARG;
    const long long al = in_bf16 ? 7 : 3;                            // rows are read as 8- / 16-byte vectors
    if (((long long)(ldq | ldk | ldv | ldkp | ldvp) | (long long)prefix_stride) & al) return VF_ERR_BAD_ARG;
    if ((lddo | lddqkv) & 3) return VF_ERR_BAD_ARG;
    const uintptr_t pal = in_bf16 ? 7 : 15;                          // ... from bases aligned likewise (a column view may start anywhere)
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)kp | (uintptr_t)vp) & pal) return VF_ERR_BAD_ARG;
    if (((uintptr_t)dout | (uintptr_t)dqkv) & 15) return VF_ERR_BAD_ARG;
    if (prefix_stride < 0) return VF_ERR_BAD_ARG;
    if (B > 65535 || N > 65535) return VF_ERR_UNSUPPORTED;           // grid dimensions y / z
    if (B == 0 || N == 0) return VF_OK;
    static unsigned long long attr_devs = 0;      // bit d: raised on device d (the attribute is per device)
    if (vf_attr_needed(&attr_devs)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_prefix_bwd_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM);
        if (e != hipSuccess) return (int)e;
        vf_attr_done(&attr_devs);
    }
    const pbwd_args a{q, k, v, kp, vp, dout, dqkv, ctx_len, C, N, H, ldq, ldk, ldv, ldkp, ldvp, lddo, lddqkv, (long long)prefix_stride,
                      in_bf16 ? 1 : 0};
    hipLaunchKernelGGL(attn_prefix_bwd_kernel, dim3((unsigned)H, (unsigned)B, (unsigned)N), dim3(NT), SMEM, (hipStream_t)stream, a);
    return vf_last_status();
}
