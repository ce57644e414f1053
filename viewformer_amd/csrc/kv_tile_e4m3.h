// One e4m3 tile of a packed context cache: the routine that vf_kv_pack_e4m3 (kv_pack.hip) and vf_kv_append_e4m3 (kv_append_e4m3.hip)
// share, so that equal tile values give equal bytes and equal scales whichever entry stored them.
//
// A workgroup of 256 threads packs one tile of 64 tokens x 64 features: thread tid loads 16 consecutive features (quarter tid & 3) of
// token tid >> 2 from `row16` — the address of those 16 elements, bf16 or fp32 —, the workgroup finds absmax, and thread tid stores
// 16 consecutive bytes of the packed tile at `dst + 16 tid`: K [key = token][feature], V [feature][key] (transposed).  Thread 0 stores
// the scale.
//
// Scale: 2^e with e the smallest integer such that absmax <= 448 * 2^e, from the exponent and mantissa FIELDS of absmax (448 = 1.75 * 2^8:
// e = ea - 8 when the mantissa is <= 1.75, else ea - 7), never from log2; e = 0 for an all-zero tile or a non-finite absmax; clamped to
// [-100, 100] so that no dequantised value is an fp32 / bf16 subnormal.  NaN elements do not enter absmax.  Elements: x * 2^-e (exact),
// clamped to +-448 by comparisons (a NaN fails both and stays NaN; the conversion itself does not saturate), then round-to-nearest-even
// by the hardware conversion.
// The tile goes through LDS as fp32 (row stride 65: the transposed read of V walks banks), so global loads and stores are whole rows.
#pragma once
#include "vf_common.h"

namespace kvt {

constexpr int PL = 64;        // tokens per view
constexpr int PD = 64;        // features per head
constexpr int PLD = PD + 1;
constexpr int TILE_FLOATS = PL * PLD;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// `tile` [TILE_FLOATS] and `wmax` [4] are the workgroup's LDS; every thread of the workgroup calls this (it synchronises once)
__device__ __forceinline__ void pack_tile_e4m3(const char* __restrict__ row16, int in16, int isv, unsigned char* __restrict__ dst,
                                               float* __restrict__ scale, float* tile, unsigned* wmax) {
    const int tid = threadIdx.x;
    const int row = tid >> 2, q4 = tid & 3;                       // token, 16-feature quarter of the head
    float x[16];
    if (in16) {
        const bf16x8* p = reinterpret_cast<const bf16x8*>(row16);
        const bf16x8 t0 = p[0], t1 = p[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) { x[j] = (float)t0[j]; x[8 + j] = (float)t1[j]; }
    } else {
        const f32x4* p = reinterpret_cast<const f32x4*>(row16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 t = p[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[4 * j + e] = t[e];
        }
    }
    unsigned am = 0;                                              // bits of the largest |x| (non-negative floats order as integers); NaN stays out
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        tile[row * PLD + q4 * 16 + j] = x[j];
        const unsigned bits = __float_as_uint(x[j]) & 0x7fffffffu;
        if (bits <= 0x7f800000u) am = max(am, bits);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) am = max(am, (unsigned)__shfl_xor((int)am, o, 64));
    if ((tid & 63) == 0) wmax[tid >> 6] = am;
    __syncthreads();
    am = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));

    int e = 0;
    if (am != 0 && am < 0x7f800000u) {
        const int ea = (int)(am >> 23) - 127;
        e = (am & 0x7fffffu) <= 0x600000u ? ea - 8 : ea - 7;
        e = min(max(e, -100), 100);
    }
    const float inv = __uint_as_float((unsigned)(127 - e) << 23);     // 2^-e, a normal number for every e in [-100, 100]
    if (tid == 0) *scale = __uint_as_float((unsigned)(127 + e) << 23);

    // thread -> 16 consecutive bytes of the packed tile: K [key = row][features 16 q4 ...], V [feature = row][keys 16 q4 ...]
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float y[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = q4 * 16 + 4 * j + t;
            const float v = (isv ? tile[i * PLD + row] : tile[row * PLD + i]) * inv;
            y[t] = v > 448.f ? 448.f : (v < -448.f ? -448.f : v);     // a NaN fails both comparisons and stays
        }
        int p = 0;
        p = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], p, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], p, true);
        w[j] = (unsigned)p;
    }
    *reinterpret_cast<uint4*>(dst + tid * 16) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace kvt
