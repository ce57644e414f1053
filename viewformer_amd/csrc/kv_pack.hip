// Pack the keys and values of a context cache to OCP e4m3 with one power-of-two scale per (scene, view, head) tile, gfx950
// (ContextCache.pack('e4m3')).
//
// The source is a layer's cache buffer as vf_kv_append takes it: [capacity * L rows][ld_src] per scene (scenes cache_stride elements apart),
// thirds (V, Q, K), bf16 or fp32.  One workgroup packs one tile of L = 64 tokens x 64 features: blockIdx.x = the view (b C + c), y = the
// head, z = 0 for the K third, 1 for the V third.  A view at or beyond lengths[b] is skipped: nothing of it is read, nothing written.
//
// The scale rule, the saturation, the NaN handling and the rounding are kv_tile_e4m3.h's (shared with vf_kv_append_e4m3).
//
// Output, tile-major, so that the prefix attention fetches a tile as one contiguous 4 KiB block (256 threads x 16 bytes):
//   kq: tile [64 keys][64 features] bytes;  vq: tile [64 features][64 keys] bytes (V already transposed: the attention's V^T image);
//   tile (b, c, h) at b * q_scene_stride + c * q_view_stride + h * 4096 bytes; its scale at b * s_scene_stride + c * s_view_stride + h.
#include "kv_tile_e4m3.h"
#include "../../include/vf_hip.h"

namespace {

using kvt::PL;
using kvt::PD;

__global__ __launch_bounds__(256) void kv_pack_e4m3_kernel(const char* __restrict__ src, int in16, unsigned char* __restrict__ kq,
                                                           unsigned char* __restrict__ vq, float* __restrict__ kscale,
                                                           float* __restrict__ vscale, unsigned C, int H, long long ld_src,
                                                           long long cache_stride, long long q_view_stride, long long q_scene_stride,
                                                           long long s_view_stride, long long s_scene_stride, const int* __restrict__ lengths) {
    __shared__ float tile[kvt::TILE_FLOATS];
    __shared__ unsigned wmax[4];

    const unsigned bc = blockIdx.x;                               // uniform in the workgroup
    const unsigned b = bc / C, c = bc - b * C;
    if ((long long)c >= (long long)lengths[b]) return;
    const int h = blockIdx.y;
    const int isv = blockIdx.z;                                   // 0: K (columns [2d, 3d)), 1: V (columns [0, d))
    const int row = threadIdx.x >> 2, q4 = threadIdx.x & 3;       // token, 16-feature quarter of the head
    const long long col = (isv ? 0LL : 2LL * H * PD) + (long long)h * PD + q4 * 16;
    const long long eoff = (long long)b * cache_stride + ((long long)c * PL + row) * ld_src + col;
    kvt::pack_tile_e4m3(src + eoff * (in16 ? 2 : 4), in16, isv,
                        (isv ? vq : kq) + (long long)b * q_scene_stride + (long long)c * q_view_stride + (long long)h * (PL * PD),
                        (isv ? vscale : kscale) + (long long)b * s_scene_stride + (long long)c * s_view_stride + h, tile, wmax);
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
