// The tail of the localization head in ONE launch (gfx950): the pose classifier's c_proj (1536 -> 7; viewformer/models/migt.py:291-292,354),
// QuaternionPoseRepresentation's output branch per token (migt.py:159-164; geometry.pose_head_postprocess) and the reduction of a view's
// L tokens to one camera (migt.py:123-129,150-154; geometry.reduce_cameras).  The inference path ran this as a GEMM whose 7 columns are
// padded to a 32-column tile plus about twenty element-wise launches on [views, L, 7] tensors: a quarter of all launches of a one-photo
// pass over a cached context (MIGT.localize_from_context).
//
//   raw     [views * L][7] = x @ W + b
//   tokens  [views * L][7] : xyz = raw.xyz / position_multiplier (IEEE division),
//                            q = raw.q * (1 / sqrt(max(sum raw.q^2, 1e-12))), then q *= (q.w >= 0 ? 1 : -1)
//   cameras [views][7]     : xyz = (sum over the view's tokens of xyz) / L,
//                            q = normalise((sum of the tokens' q) / L), then sign-fixed the same way
//
// Shape.  One 256-thread workgroup per view.  W^T is staged once per workgroup in LDS as [8][K] (as dense_small_n_kernel in train_ops.hip:
// a lane's float4 reads of one output's weights are contiguous); one wave per token row, lanes stride K in float4 steps with seven
// accumulators, vf_wave_sum_dpp for the row sums; lane 0 post-processes the token and leaves it in an LDS [L][7] array.  After one
// barrier wave 0 reduces the view from that array by a FIXED schedule in token order: lane l adds the tokens l, l + 64, l + 128, l + 192
// in that order, and the 64 partial sums meet in vf_wave_sum_dpp's fixed order.  No atomics, nothing depends on `views` or on
// blockIdx beyond the choice of rows: a view's three outputs are bit-identical whatever else the launch holds, and whichever of the
// optional outputs are requested.
//
// Arithmetic.  fp32.  The dot products are fmaf chains (k ascending within a lane, lanes by the DPP schedule); everything after them is
// explicitly rounded operation by operation (no contraction), sums of squares left to right.
//
// LDS: 8 * K * 4 bytes of weights + L * 7 * 4 bytes of tokens (rounded up to 16), all in the dynamic region (64 KiB + 7 KiB at K = 2048,
// L = 256).  No static LDS: the dynamic base stays 16-byte aligned for the float4 reads.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_WAVES = PT_THREADS / VF_WAVE;
constexpr int PT_N = 7;                 // xyz + quaternion (w, x, y, z)
constexpr int PT_ROWS = 8;              // rows of the staged W^T (row 7 is zero and never read)
constexpr int PT_MAX_K = 2048;
constexpr int PT_MAX_L = 256;

// tf.math.l2_normalize's factor: 1 / sqrt(max(sum x^2, 1e-12)) (geometry.quaternion_normalize)
__device__ __forceinline__ float pt_inv_norm4(float w, float x, float y, float z) {
    const float ss = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w, w), __fmul_rn(x, x)), __fmul_rn(y, y)), __fmul_rn(z, z));
    return __fdiv_rn(1.0f, __fsqrt_rn(fmaxf(ss, 1e-12f)));
}

// q <- remove_sign(normalize(q)), in place (geometry.quaternion_normalize, quaternion_remove_sign)
__device__ __forceinline__ void pt_unit_quaternion(float* q) {
    const float inv = pt_inv_norm4(q[0], q[1], q[2], q[3]);
    const float w = __fmul_rn(q[0], inv);
    const float s = w >= 0.0f ? 1.0f : -1.0f;
    q[0] = __fmul_rn(w, s);
    q[1] = __fmul_rn(__fmul_rn(q[1], inv), s);
    q[2] = __fmul_rn(__fmul_rn(q[2], inv), s);
    q[3] = __fmul_rn(__fmul_rn(q[3], inv), s);
}

__global__ __launch_bounds__(PT_THREADS) void pose_tail_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ W,
                                                               const float* __restrict__ b, float position_multiplier, int L, int K,
                                                               float* __restrict__ raw, float* __restrict__ tokens, float* __restrict__ cameras) {
    extern __shared__ __attribute__((aligned(16))) float pt_smem[];
    float* wt = pt_smem;                          // [PT_ROWS][K]: W transposed
    float* tok = pt_smem + PT_ROWS * K;           // [L][PT_N]: the view's post-processed tokens
    for (int i = threadIdx.x; i < PT_ROWS * K; i += PT_THREADS) {
        const int n = i / K, k = i - n * K;
        wt[i] = n < PT_N ? W[(size_t)k * PT_N + n] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & (VF_WAVE - 1), wave = threadIdx.x / VF_WAVE;
    const int k4 = K >> 2;
    const long long view = blockIdx.x;
    for (int t = wave; t < L; t += PT_WAVES) {
        const long long r = view * L + t;
        const f32x4* __restrict__ xr = reinterpret_cast<const f32x4*>(x + r * ldx);
        float acc[PT_N];
#pragma unroll
        for (int n = 0; n < PT_N; ++n) acc[n] = 0.f;
        for (int c = lane; c < k4; c += VF_WAVE) {
            const f32x4 xv = xr[c];
#pragma unroll
            for (int n = 0; n < PT_N; ++n) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + n * K + 4 * c);
                acc[n] = __builtin_fmaf(xv[0], wv[0], __builtin_fmaf(xv[1], wv[1], __builtin_fmaf(xv[2], wv[2], __builtin_fmaf(xv[3], wv[3], acc[n]))));
            }
        }
#pragma unroll
        for (int n = 0; n < PT_N; ++n) acc[n] = vf_wave_sum_dpp(acc[n]);
        if (lane == 0) {
#pragma unroll
            for (int n = 0; n < PT_N; ++n) acc[n] = __fadd_rn(acc[n], b ? b[n] : 0.f);
            if (raw) {
#pragma unroll
                for (int n = 0; n < PT_N; ++n) raw[r * PT_N + n] = acc[n];
            }
#pragma unroll
            for (int n = 0; n < 3; ++n) acc[n] = __fdiv_rn(acc[n], position_multiplier);
            pt_unit_quaternion(acc + 3);
#pragma unroll
            for (int n = 0; n < PT_N; ++n) tok[t * PT_N + n] = acc[n];
            if (tokens) {
#pragma unroll
                for (int n = 0; n < PT_N; ++n) tokens[r * PT_N + n] = acc[n];
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
        float s[PT_N];
#pragma unroll
        for (int n = 0; n < PT_N; ++n) s[n] = 0.f;
        for (int t = lane; t < L; t += VF_WAVE) {
#pragma unroll
            for (int n = 0; n < PT_N; ++n) s[n] = __fadd_rn(s[n], tok[t * PT_N + n]);
        }
#pragma unroll
        for (int n = 0; n < PT_N; ++n) s[n] = vf_wave_sum_dpp(s[n]);
        if (lane == 0) {
#pragma unroll
            for (int n = 0; n < PT_N; ++n) s[n] = __fdiv_rn(s[n], (float)L);
            pt_unit_quaternion(s + 3);
#pragma unroll
            for (int n = 0; n < PT_N; ++n) cameras[view * PT_N + n] = s[n];
        }
    }
}

}  // namespace

extern "C" {

int vf_pose_tail_f32(const float* x, int64_t ldx, const float* W, const float* b, float position_multiplier, int64_t views, int L, int K,
                     float* raw, float* tokens, float* cameras, void* stream) {
    if (!x || !W || !cameras || views < 0 || K <= 0 || ldx < K || (reinterpret_cast<uintptr_t>(x) & 15)) return VF_ERR_BAD_ARG;
    if (!(position_multiplier != 0.0f) || !(fabsf(position_multiplier) < __builtin_inff())) return VF_ERR_BAD_ARG;
    if ((K & 3) || K < 4 || K > PT_MAX_K || L < 1 || L > PT_MAX_L || (ldx & 3) || views > 0x7fffffffll) return VF_ERR_UNSUPPORTED;
    if (views == 0) return VF_OK;
    const size_t smem = ((size_t)PT_ROWS * K + (((size_t)L * PT_N + 3) & ~(size_t)3)) * sizeof(float);
    static unsigned long long attr_devs = 0;
    if (smem > 64 * 1024 && vf_attr_needed(&attr_devs)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pose_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        if (e != hipSuccess) return (int)e;
        vf_attr_done(&attr_devs);
    }
    hipLaunchKernelGGL(pose_tail_kernel, dim3((unsigned)views), dim3(PT_THREADS), smem, (hipStream_t)stream, x, (long long)ldx, W, b,
                       position_multiplier, L, K, raw, tokens, cameras);
    return vf_last_status();
}

}  // extern "C"
