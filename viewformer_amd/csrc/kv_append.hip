// Append the keys and values of new views to a context cache with room: one launch per layer for every scene of a ragged batch, gfx950.
//
// The cache of a layer is [capacity * L rows][ld_dst] per scene (scenes cache_stride elements apart), rows in the layout of the fused c_attn
// output: thirds (V, Q, K).  qkv is that output for K new views per scene, rows [B*K*L][ld_src].  New view j of scene b goes to the cache's
// view pos[b] + j: its V third (columns [0, d)) and its K third (columns [2d, 3d)) are copied, bit for bit; the Q third of a cached view is
// never read again and is not written.  pos lives on the device (each scene's own length), so a roll-out needs no host round trip.  A view
// whose slot falls outside [0, capacity) is skipped (the attention clamps its lengths the same way; the host never asks for it).
//
// Grid: x = the new view (b K + j), y = a slice of that view's work.  Scene, view number and slot are uniform in a workgroup (one read of
// pos, one 32-bit division, an early exit for a skipped view).  The unit of work is one 16-byte chunk: d * elem_bytes / 16 chunks per third,
// two thirds per row, L rows per view; a thread takes chunks of its view stride by stride (one 32-bit division each), consecutive threads
// consecutive chunks of a row's third, so a wave's loads and stores are whole runs of up to 1 KiB.  At B = 16, K = 1, d = 768 the launch
// moves about 3 MB each way: launch latency, not bandwidth, is its cost.  Small launches take 64-thread blocks so that
// their few thousand chunks still spread over the CUs; large ones (a cache that moves to bigger buffers) are capped at about 8192 blocks.
//
// vf_kv_append_split is the same loop for a cache that holds no Q third (a growing K/V-only cache): one destination per third.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

// SPLIT (vf_kv_append_split, a growing K/V-only cache): the same loop with a destination per third — the V third to
// rows of `dst` (leading dimension ld_dst, column 0), the K third to rows of `dstk` (ld_k, column 0), each with its own scene stride.
template <bool SPLIT>
__global__ void kv_append_kernel(const char* __restrict__ src, char* __restrict__ dst, char* __restrict__ dstk, unsigned chunks, unsigned cpr,
                                 unsigned K, unsigned L, long long third_bytes, long long ld_src_bytes, long long ld_dst_bytes,
                                 long long stride_bytes, long long ld_k_bytes, long long stride_k_bytes, int capacity,
                                 const int* __restrict__ pos) {
    const unsigned bj = blockIdx.x;                               // new view b K + j: uniform in the workgroup
    const unsigned b = bj / K, j = bj - b * K;
    const long long view = (long long)pos[b] + j;
    if (view < 0 || view >= capacity) return;
    const char* s = src + (long long)bj * L * ld_src_bytes;
    char* t = dst + b * stride_bytes + view * L * ld_dst_bytes;
    char* tk = SPLIT ? dstk + b * stride_k_bytes + view * L * ld_k_bytes : nullptr;
    for (unsigned i = blockIdx.y * blockDim.x + threadIdx.x; i < chunks; i += gridDim.y * blockDim.x) {
        const unsigned l = i / (2 * cpr), c = i - l * (2 * cpr);  // row of the view, chunk of the row's two thirds
        const unsigned third = c >= cpr;                          // 0: V at column 0, 1: K at column 2d
        const long long in = (long long)(c - third * cpr) * 16;   // byte inside the third
        const uint4 x = *reinterpret_cast<const uint4*>(s + l * ld_src_bytes + third * third_bytes + in);
        if (SPLIT)
            *reinterpret_cast<uint4*>(third ? tk + l * ld_k_bytes + in : t + l * ld_dst_bytes + in) = x;
        else
            *reinterpret_cast<uint4*>(t + l * ld_dst_bytes + third * third_bytes + in) = x;
    }
}

// grid and block of both entries: small launches take 64-thread blocks, large ones are capped at about 8192 blocks
template <bool SPLIT>
int launch(const void* qkv, void* dst, void* dstk, long long views, long long chunks, long long cpr, int K, int L, long long third_bytes,
           long long ld_src_bytes, long long ld_dst_bytes, long long stride_bytes, long long ld_k_bytes, long long stride_k_bytes, int capacity,
           const int32_t* pos, void* stream) {
    const int threads = views * chunks < 256LL * 256 ? 64 : 256;  // fewer than one 256-thread block per CU: smaller blocks, more CUs
    long long slices = (chunks + threads - 1) / threads;
    const long long cap = views >= 8192 ? 1 : 8192 / views;      // about 8192 blocks at the most: the threads stride over the rest
    if (slices > cap) slices = cap;
    hipLaunchKernelGGL(kv_append_kernel<SPLIT>, dim3((unsigned)views, (unsigned)slices), dim3(threads), 0, (hipStream_t)stream,
                       (const char*)qkv, (char*)dst, (char*)dstk, (unsigned)chunks, (unsigned)cpr, (unsigned)K, (unsigned)L, third_bytes,
                       ld_src_bytes, ld_dst_bytes, stride_bytes, ld_k_bytes, stride_k_bytes, capacity, reinterpret_cast<const int*>(pos));
    return vf_last_status();
}

}  // namespace

extern "C" {

int vf_kv_append(const void* qkv, void* cache, int elem_bytes, int B, int K, int L, int d, int ld_src, int ld_dst, int64_t cache_stride,
                 int capacity, const int32_t* pos, void* stream) {
    if (!qkv || !cache || !pos) return VF_ERR_BAD_ARG;
    if (elem_bytes != 2 && elem_bytes != 4) return VF_ERR_BAD_ARG;
    if (B < 0 || K < 0 || L < 0 || d < 0 || capacity < 0 || cache_stride < 0) return VF_ERR_BAD_ARG;
    if (ld_src < 3LL * d || ld_dst < 3LL * d) return VF_ERR_BAD_ARG;
    if (((long long)d * elem_bytes) % 16 || ((long long)ld_src * elem_bytes) % 16 || ((long long)ld_dst * elem_bytes) % 16 ||
        ((long long)cache_stride * elem_bytes) % 16)
        return VF_ERR_BAD_ARG;
    if (((uintptr_t)qkv | (uintptr_t)cache) & 15) return VF_ERR_BAD_ARG;
    if (B > 1 && capacity > 0 && L > 0 && cache_stride < ((long long)capacity * L - 1) * ld_dst + 3LL * d) return VF_ERR_BAD_ARG;   // scenes would overlap
    const long long views = (long long)B * K;
    const long long cpr = (long long)d * elem_bytes / 16;
    const long long chunks = (long long)L * 2 * cpr;             // per view
    if (views > 0x7fffffffLL || chunks > 0x7fffffffLL) return VF_ERR_UNSUPPORTED;
    if (views == 0 || chunks == 0 || capacity == 0) return VF_OK;
    return launch<false>(qkv, cache, nullptr, views, chunks, cpr, K, L, 2LL * d * elem_bytes, (long long)ld_src * elem_bytes,
                         (long long)ld_dst * elem_bytes, (long long)cache_stride * elem_bytes, 0, 0, capacity, pos, stream);
}

int vf_kv_append_split(const void* qkv, void* k, void* v, int elem_bytes, int B, int K, int L, int d, int ld_src, int ld_k, int ld_v,
                       int64_t k_stride, int64_t v_stride, int capacity, const int32_t* pos, void* stream) {
    if (!qkv || !k || !v || !pos) return VF_ERR_BAD_ARG;
    if (elem_bytes != 2 && elem_bytes != 4) return VF_ERR_BAD_ARG;
    if (B < 0 || K < 0 || L < 0 || d < 0 || capacity < 0 || k_stride < 0 || v_stride < 0) return VF_ERR_BAD_ARG;
    if (ld_src < 3LL * d || ld_k < d || ld_v < d) return VF_ERR_BAD_ARG;
    if (((long long)d * elem_bytes) % 16 || ((long long)ld_src * elem_bytes) % 16 || ((long long)ld_k * elem_bytes) % 16 ||
        ((long long)ld_v * elem_bytes) % 16 || ((long long)k_stride * elem_bytes) % 16 || ((long long)v_stride * elem_bytes) % 16)
        return VF_ERR_BAD_ARG;
    if (((uintptr_t)qkv | (uintptr_t)k | (uintptr_t)v) & 15) return VF_ERR_BAD_ARG;
    if (B > 1 && capacity > 0 && L > 0 && (k_stride < ((long long)capacity * L - 1) * ld_k + d || v_stride < ((long long)capacity * L - 1) * ld_v + d))
        return VF_ERR_BAD_ARG;                                    // scenes would overlap
    const long long views = (long long)B * K;
    const long long cpr = (long long)d * elem_bytes / 16;
    const long long chunks = (long long)L * 2 * cpr;             // per view
    if (views > 0x7fffffffLL || chunks > 0x7fffffffLL) return VF_ERR_UNSUPPORTED;
    if (views == 0 || chunks == 0 || capacity == 0) return VF_OK;
    return launch<true>(qkv, v, k, views, chunks, cpr, K, L, 2LL * d * elem_bytes, (long long)ld_src * elem_bytes, (long long)ld_v * elem_bytes,
                        (long long)v_stride * elem_bytes, (long long)ld_k * elem_bytes, (long long)k_stride * elem_bytes, capacity, pos, stream);
}

}  // extern "C"
