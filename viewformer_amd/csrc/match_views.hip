// Many photos against many cameras: the [B][M][P] log-likelihood matrix from M scored views, gfx950.
//
// A scored view is a MASK view: its logits, lse and arg-max depend on the context and the camera only; the photo enters after the LM head,
// as the index of a gather.  So P photos against M cameras need the M views' logits once (vf_gemm / vf_logits_score_f32) and, per
// (camera, photo), what vf_score_views_f32 does for one pair: x_t = logits[row_t][code_t] - lse[row_t] (-inf for a code outside [0, V),
// for which nothing is read) summed as ONE fp32 chain in token order, and the share of tokens whose arg-max is the photo's code.
//
// One workgroup = one (scene, camera) x a tile of 256 photos, one thread per photo: the thread runs its photo's token chain, which gives the
// token order for free and makes an element a function of its own (b, m, p) inputs alone — no atomics, no workspace, no cross-lane sum.
// The photos' codes ([photo][token] in memory, so a thread's own codes are L ints apart from its neighbour's) are staged through LDS in slabs
// of 32 tokens: the workgroup reads each photo's 128-byte piece of the slab with consecutive lanes and every thread then reads its own row
// of the slab (row pitch 33 dwords: lanes of a wave fall on different banks).  lse and idx of a token are the same address for the whole
// workgroup.  The logits are gathered from global memory: the view's L rows (L x V x 4 bytes, 256 KB at 64 x 1024) are read by every photo
// tile of that (scene, camera), and vf_xcd_bid() keeps the tiles of one view on one XCD, so the view is fetched into that L2 once and the
// gathers hit there.  Staging the view's rows in LDS instead (160 KB: slabs of at most 32 rows of 1024 codes) would replace each 4-byte L2
// gather by an LDS read, at the price of streaming the whole view through every photo tile's workgroup — 256 KB of loads per 256 x 64
// gathered elements (64 KB) — so it only pays once L2 gather latency, not bytes, bounds the kernel; not built.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

constexpr int TP = 256;                   // photos per workgroup, one thread each
constexpr int TS = 32;                    // tokens per staged slab of codes
constexpr int PITCH = TS + 1;             // dwords per photo row of the slab
constexpr int TG = 8;                     // gathers a thread keeps in flight

__global__ __launch_bounds__(256) void match_views_kernel(const float* __restrict__ logits, long long ld, const float* __restrict__ lse,
                                                          const long long* __restrict__ idx, const int* __restrict__ codes,
                                                          long long scene_stride, long long M, long long P, int L, int V, unsigned tiles,
                                                          float* __restrict__ ll, float* __restrict__ acc) {
    __shared__ int slab[TP * PITCH];
    const int tid = threadIdx.x;
    const unsigned bid = vf_xcd_bid();                                      // the photo tiles of one view on one XCD
    const long long bm = bid / tiles;                                       // b * M + m
    const long long p0 = (long long)(bid % tiles) * TP;
    const int np = P - p0 < TP ? (int)(P - p0) : TP;                        // photos of this tile, >= 1
    const int* cb = codes + (bm / M) * scene_stride + p0 * L;
    const long long row0 = bm * L;
    float sum = 0.f;
    int hits = 0;
    for (int t0 = 0; t0 < L; t0 += TS) {
        const int ts = L - t0 < TS ? L - t0 : TS;
        if (t0) __syncthreads();                                            // the previous slab has been read
        for (int i = tid; i < np * ts; i += 256) {                          // consecutive lanes: consecutive tokens of a photo
            const int pp = i / ts, tt = i - pp * ts;
            slab[pp * PITCH + tt] = cb[(long long)pp * L + t0 + tt];
        }
        __syncthreads();
        if (tid < np) {
            for (int g0 = 0; g0 < ts; g0 += TG) {                             // TG gathers in flight, then their links of the chain in token order
                int c[TG];
                float z[TG];
#pragma unroll
                for (int j = 0; j < TG; ++j) {
                    c[j] = g0 + j < ts ? slab[tid * PITCH + g0 + j] : -1;
                    z[j] = 0.f;
                    if ((unsigned)c[j] < (unsigned)V) z[j] = logits[(row0 + t0 + g0 + j) * ld + c[j]];       // nothing is read for a code outside [0, V)
                }
#pragma unroll
                for (int j = 0; j < TG; ++j) {
                    if (g0 + j < ts) {
                        const long long row = row0 + t0 + g0 + j;
                        const float x = (unsigned)c[j] < (unsigned)V ? __fsub_rn(z[j], lse[row]) : -INFINITY;
                        sum = (t0 + g0 + j) ? __fadd_rn(sum, x) : x;
                        if (acc) hits += idx[row] == (long long)c[j];
                    }
                }
            }
        }
    }
    if (tid < np) {
        const long long o = bm * P + p0 + tid;
        ll[o] = sum;
        if (acc) acc[o] = (float)hits / (float)L;
    }
}

}  // namespace

extern "C" {

int vf_match_views_f32(const float* logits, int64_t ld, const float* lse, const int64_t* idx, const int32_t* codes, int64_t codes_scene_stride,
                       int64_t B, int64_t M, int64_t P, int L, int V, float* log_likelihood, float* accuracy, void* stream) {
    if (!logits || !lse || !codes || !log_likelihood || (accuracy && !idx)) return VF_ERR_BAD_ARG;
    if (B < 0 || M < 0 || P < 0 || L <= 0 || V <= 0 || ld < V) return VF_ERR_BAD_ARG;
    if (codes_scene_stride < 0 || (codes_scene_stride > 0 && codes_scene_stride / L < P)) return VF_ERR_BAD_ARG;       // 0 < stride < P * L
    if (B == 0 || M == 0 || P == 0) return VF_OK;
    const int64_t tiles = (P - 1) / TP + 1;
    if (B > 0x7fffffffLL / M || B * M > 0x7fffffffLL / tiles) return VF_ERR_UNSUPPORTED;            // the grid's x dimension
    hipLaunchKernelGGL(match_views_kernel, dim3((unsigned)(B * M * tiles)), dim3(256), 0, (hipStream_t)stream, logits, (long long)ld, lse,
                       reinterpret_cast<const long long*>(idx), reinterpret_cast<const int*>(codes), (long long)codes_scene_stride, (long long)M,
                       (long long)P, L, V, (unsigned)tiles, log_likelihood, accuracy);
    return vf_last_status();
}

}  // extern "C"
