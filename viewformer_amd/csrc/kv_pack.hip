// Pack the keys and values of a context cache to OCP e4m3 with one power-of-two scale per (scene, view, head) tile, gfx950
// (ContextCache.pack('e4m3')).
//
// The source is a layer's cache buffer as vf_kv_append takes it: [capacity * L rows][ld_src] per scene (scenes cache_stride elements apart),
// thirds (V, Q, K), bf16 or fp32.  One workgroup packs one tile of L = 64 tokens x 64 features: blockIdx.x = the view (b C + c), y = the
// head, z = 0 for the K third, 1 for the V third.  A view at or beyond lengths[b] is skipped: nothing of it is read, nothing written.
//
// Scale: 2^e with e the smallest integer such that absmax <= 448 * 2^e, from the exponent and mantissa FIELDS of absmax (448 = 1.75 * 2^8:
// e = ea - 8 when the mantissa is <= 1.75, else ea - 7), never from log2; e = 0 for an all-zero tile or a non-finite absmax; clamped to
// [-100, 100] so that no dequantised value is an fp32 / bf16 subnormal.  NaN elements do not enter absmax.  Elements: x * 2^-e (exact),
// clamped to +-448 by comparisons (a NaN fails both and stays NaN; the conversion itself does not saturate), then round-to-nearest-even
// by the hardware conversion.
//
// Output, tile-major, so that the prefix attention fetches a tile as one contiguous 4 KiB block (256 threads x 16 bytes):
//   kq: tile [64 keys][64 features] bytes;  vq: tile [64 features][64 keys] bytes (V already transposed: the attention's V^T image);
//   tile (b, c, h) at b * q_scene_stride + c * q_view_stride + h * 4096 bytes; its scale at b * s_scene_stride + c * s_view_stride + h.
// The tile goes through LDS as fp32 (row stride 65: the transposed read of V walks banks), so global loads and stores are whole rows.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

constexpr int PL = 64;        // tokens per view
constexpr int PD = 64;        // features per head
constexpr int PLD = PD + 1;

typedef __bf16 pk_bf16x8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(256) void kv_pack_e4m3_kernel(const char* __restrict__ src, int in16, unsigned char* __restrict__ kq,
                                                           unsigned char* __restrict__ vq, float* __restrict__ kscale,
                                                           float* __restrict__ vscale, unsigned C, int H, long long ld_src,
                                                           long long cache_stride, long long q_view_stride, long long q_scene_stride,
                                                           long long s_view_stride, long long s_scene_stride, const int* __restrict__ lengths) {
    __shared__ float tile[PL * PLD];
    __shared__ unsigned wmax[4];

    const unsigned bc = blockIdx.x;                               // uniform in the workgroup
    const unsigned b = bc / C, c = bc - b * C;
    if ((long long)c >= (long long)lengths[b]) return;
    const int h = blockIdx.y;
    const int isv = blockIdx.z;                                   // 0: K (columns [2d, 3d)), 1: V (columns [0, d))
    const int tid = threadIdx.x;
    const int row = tid >> 2, q4 = tid & 3;                       // token, 16-feature quarter of the head
    const long long col = (isv ? 0LL : 2LL * H * PD) + (long long)h * PD + q4 * 16;
    const long long eoff = (long long)b * cache_stride + ((long long)c * PL + row) * ld_src + col;

    float x[16];
    if (in16) {
        const pk_bf16x8* p = reinterpret_cast<const pk_bf16x8*>(src + eoff * 2);
        const pk_bf16x8 t0 = p[0], t1 = p[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) { x[j] = (float)t0[j]; x[8 + j] = (float)t1[j]; }
    } else {
        const f32x4* p = reinterpret_cast<const f32x4*>(src + eoff * 4);
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
    if (tid == 0) {
        const long long so = (long long)b * s_scene_stride + (long long)c * s_view_stride + h;
        (isv ? vscale : kscale)[so] = __uint_as_float((unsigned)(127 + e) << 23);
    }

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
    unsigned char* dst = (isv ? vq : kq) + (long long)b * q_scene_stride + (long long)c * q_view_stride + (long long)h * (PL * PD) + tid * 16;
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

extern "C" {

int vf_kv_pack_e4m3(const void* cache, int elem_bytes, void* kq, void* vq, float* kscale, float* vscale, int B, int C, int H, int L,
                    int ld_src, int64_t cache_stride, int64_t q_view_stride, int64_t q_scene_stride, int64_t s_view_stride,
                    int64_t s_scene_stride, const int32_t* lengths, void* stream) {
    if (!cache || !kq || !vq || !kscale || !vscale || !lengths) return VF_ERR_BAD_ARG;
    if (elem_bytes != 2 && elem_bytes != 4) return VF_ERR_BAD_ARG;
    if (B < 0 || C < 0 || H <= 0 || L < 0 || cache_stride < 0) return VF_ERR_BAD_ARG;
    if (L != PL) return VF_ERR_UNSUPPORTED;
    if (ld_src < 3LL * H * PD) return VF_ERR_BAD_ARG;
    if (((long long)ld_src * elem_bytes) % 16 || ((long long)cache_stride * elem_bytes) % 16) return VF_ERR_BAD_ARG;
    if (((uintptr_t)cache | (uintptr_t)kq | (uintptr_t)vq) & 15) return VF_ERR_BAD_ARG;
    if (((uintptr_t)kscale | (uintptr_t)vscale) & 3) return VF_ERR_BAD_ARG;
    if (q_view_stride < (long long)H * PL * PD || q_scene_stride < 0 || (q_view_stride | q_scene_stride) & 15) return VF_ERR_BAD_ARG;
    if (s_view_stride < H || s_scene_stride < 0) return VF_ERR_BAD_ARG;
    if (B > 1 && C > 0 && (q_scene_stride < (long long)(C - 1) * q_view_stride + (long long)H * PL * PD ||
                           s_scene_stride < (long long)(C - 1) * s_view_stride + H ||
                           cache_stride < ((long long)C * L - 1) * ld_src + 3LL * H * PD))
        return VF_ERR_BAD_ARG;                                    // scenes would overlap
    if ((long long)B * C > 0x7fffffffLL || H > 65535) return VF_ERR_UNSUPPORTED;
    if (B == 0 || C == 0) return VF_OK;
    hipLaunchKernelGGL(kv_pack_e4m3_kernel, dim3((unsigned)((long long)B * C), (unsigned)H, 2), dim3(256), 0, (hipStream_t)stream,
                       (const char*)cache, elem_bytes == 2 ? 1 : 0, (unsigned char*)kq, (unsigned char*)vq, kscale, vscale, (unsigned)C, H,
                       (long long)ld_src, (long long)cache_stride, (long long)q_view_stride, (long long)q_scene_stride,
                       (long long)s_view_stride, (long long)s_scene_stride, reinterpret_cast<const int*>(lengths));
    return vf_last_status();
}

}  // extern "C"
