// Append the keys and values of new views to an e4m3-packed context cache with room: the quantising form of vf_kv_append, one launch
// per layer for every scene of a ragged batch, gfx950 (a growing PackedE4M3Cache).
//
// qkv is the fused c_attn output of K new views per scene, rows [B*K*L][ld_src], thirds (V, Q, K), bf16 or fp32.  New view j of scene b
// goes to slot pos[b] + j of the packed buffers, addressed as vf_kv_pack_e4m3 addresses them: tile (b, slot, h) at byte
// b * q_scene_stride + slot * q_view_stride + h * 4096 of kq ([64 keys][64 features]) and of vq ([64 features][64 keys], V transposed), its
// scale at element b * s_scene_stride + slot * s_view_stride + h.  pos lives on the device (each scene's own length), so a roll-out needs
// no host round trip.  A view whose slot falls outside [0, capacity) is skipped: nothing of it is read, nothing written (vf_kv_append's
// clamp).  A new view brings its own tiles and scales: nothing that is stored already is read, re-quantised or written.
//
// Grid: x = the new view (b K + j), y = the head, z = 0 for the K third, 1 for the V third: one workgroup of 256 threads per tile, the
// tile routine of kv_tile_e4m3.h (the one vf_kv_pack_e4m3 runs: equal values give equal bytes and scales).  Scene, view number and slot
// are uniform in a workgroup (one read of pos, one 32-bit division, an early exit for a skipped view).
#include "kv_tile_e4m3.h"
#include "../../include/vf_hip.h"

namespace {

using kvt::PL;
using kvt::PD;

__global__ __launch_bounds__(256) void kv_append_e4m3_kernel(const char* __restrict__ src, int in16, unsigned char* __restrict__ kq,
                                                             unsigned char* __restrict__ vq, float* __restrict__ kscale,
                                                             float* __restrict__ vscale, unsigned K, int H, long long ld_src,
                                                             long long q_view_stride, long long q_scene_stride, long long s_view_stride,
                                                             long long s_scene_stride, int capacity, const int* __restrict__ pos) {
    __shared__ float tile[kvt::TILE_FLOATS];
    __shared__ unsigned wmax[4];

    const unsigned bj = blockIdx.x;                               // new view b K + j: uniform in the workgroup
    const unsigned b = bj / K, j = bj - b * K;
    const long long slot = (long long)pos[b] + j;
    if (slot < 0 || slot >= capacity) return;
    const int h = blockIdx.y;
    const int isv = blockIdx.z;                                   // 0: K (columns [2d, 3d)), 1: V (columns [0, d))
    const int row = threadIdx.x >> 2, q4 = threadIdx.x & 3;       // token, 16-feature quarter of the head
    const long long col = (isv ? 0LL : 2LL * H * PD) + (long long)h * PD + q4 * 16;
    const long long eoff = ((long long)bj * PL + row) * ld_src + col;
    kvt::pack_tile_e4m3(src + eoff * (in16 ? 2 : 4), in16, isv,
                        (isv ? vq : kq) + (long long)b * q_scene_stride + slot * q_view_stride + (long long)h * (PL * PD),
                        (isv ? vscale : kscale) + (long long)b * s_scene_stride + slot * s_view_stride + h, tile, wmax);
}

}  // namespace

extern "C" {

int vf_kv_append_e4m3(const void* qkv, int elem_bytes, void* kq, void* vq, float* kscale, float* vscale, int B, int K, int H, int L,
                      int ld_src, int64_t q_view_stride, int64_t q_scene_stride, int64_t s_view_stride, int64_t s_scene_stride,
                      int capacity, const int32_t* pos, void* stream) {
    if (!qkv || !kq || !vq || !kscale || !vscale || !pos) return VF_ERR_BAD_ARG;
    if (elem_bytes != 2 && elem_bytes != 4) return VF_ERR_BAD_ARG;
    if (B < 0 || K < 0 || H <= 0 || L < 0 || capacity < 0) return VF_ERR_BAD_ARG;
    if (L != PL) return VF_ERR_UNSUPPORTED;
    if (ld_src < 3LL * H * PD) return VF_ERR_BAD_ARG;
    if (((long long)ld_src * elem_bytes) % 16) return VF_ERR_BAD_ARG;
    if (((uintptr_t)qkv | (uintptr_t)kq | (uintptr_t)vq) & 15) return VF_ERR_BAD_ARG;
    if (((uintptr_t)kscale | (uintptr_t)vscale) & 3) return VF_ERR_BAD_ARG;
    if (q_view_stride < (long long)H * PL * PD || q_scene_stride < 0 || (q_view_stride | q_scene_stride) & 15) return VF_ERR_BAD_ARG;
    if (s_view_stride < H || s_scene_stride < 0) return VF_ERR_BAD_ARG;
    if (B > 1 && capacity > 0 && (q_scene_stride < (long long)(capacity - 1) * q_view_stride + (long long)H * PL * PD ||
                                  s_scene_stride < (long long)(capacity - 1) * s_view_stride + H))
        return VF_ERR_BAD_ARG;                                    // scenes would overlap
    if ((long long)B * K > 0x7fffffffLL || H > 65535) return VF_ERR_UNSUPPORTED;
    if (B == 0 || K == 0 || capacity == 0) return VF_OK;
    hipLaunchKernelGGL(kv_append_e4m3_kernel, dim3((unsigned)((long long)B * K), (unsigned)H, 2), dim3(256), 0, (hipStream_t)stream,
                       (const char*)qkv, elem_bytes == 2 ? 1 : 0, (unsigned char*)kq, (unsigned char*)vq, kscale, vscale, (unsigned)K, H,
                       (long long)ld_src, (long long)q_view_stride, (long long)q_scene_stride, (long long)s_view_stride,
                       (long long)s_scene_stride, capacity, reinterpret_cast<const int*>(pos));
    return vf_last_status();
}

}  // extern "C"
