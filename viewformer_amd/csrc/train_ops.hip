// Training-step kernels of the MIGT transformer, gfx950, fp32.
//
// The dense contractions of the backward pass reuse igemm_f32.hip (dX = dY.W^T with the weight packed
// transposed; dW = X^T.dY through vf_transpose_f32 + a packed dY).  This file holds the HBM-bound pieces:
// transposes, column sums (bias grads), LayerNorm backward, exact-erf GELU forward/backward, the
// materialised branching-attention softmax (forward with the reference's w*m - 1e4*(1-m) mask and its
// backward), softmax-cross-entropy, the pose MSE, the embedding backward and the AdamWeightDecay update.
// Reference: MIGT.train_step migt.py:464-505, losses :416-448, QuaternionPoseRepresentation.call :156-177,
// AdamWeightDecay / WarmUp / create_optimizer viewformer/models/utils.py:310-564.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

inline unsigned grid1(long long total, int per_block, unsigned cap = 32768) {
    long long b = (total + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// ------------------------------------------------------------------ batched 2-D transpose (32x32 LDS tiles)
template <typename TS>          // TS = float, or __bf16 (a saved bf16 activation widened on the way: exact)
__global__ __launch_bounds__(256) void transpose_kernel(const TS* __restrict__ src, float* __restrict__ dst, int rows,
                                                        int cols, long long ld_src, long long ld_dst,
                                                        long long bs_src, long long bs_dst) {
    __shared__ float tile[32][33];
    const TS* s = src + blockIdx.z * bs_src;
    float* d = dst + blockIdx.z * bs_dst;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        tile[ty + 8 * i][tx] = (r < rows && c < cols) ? (float)s[(long long)r * ld_src + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;          // dst[c][r]
        if (c < cols && r < rows) d[(long long)c * ld_dst + r] = tile[tx][ty + 8 * i];
    }
}

// ------------------------------------------------------------------ column sums: out[n] (+)= sum_m x[m][n]
// stage 1: grid (ceil(N/256), nsplit) -> part[split][N]; stage 2 reduces the splits in fixed order (deterministic)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, float* __restrict__ part, long long M,
                                                             int N, long long ld, int nsplit) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long per = (M + nsplit - 1) / nsplit;
    const long long m0 = blockIdx.y * per, m1 = min(M, m0 + per);
    float s = 0.f;
    for (long long m = m0; m < m1; ++m) s += x[m * ld + n];
    part[(long long)blockIdx.y * N + n] = s;
}
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ part, float* __restrict__ out, int N,
                                                           int nsplit, int accumulate) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int i = 0; i < nsplit; ++i) s += part[(long long)i * N + n];
    out[n] = accumulate ? out[n] + s : s;
}

// stage 1 for wide matrices (vf_colsum_f32): float4 columns, four row phases per block combined in a fixed order.  (A one-launch form in
// which the last block of a column block to finish — an integer ticket — folded the slabs was tried in round 3 and REMOVED: the
// device-scope fence it needs between the slab writes and the ticket makes every block write its XCD's L2 back (8 XCDs, 8 L2s), and the
// launch took 158 us on average where these two take 30-45 + 17.)
__global__ __launch_bounds__(256) void colsum_partial4_kernel(const float* __restrict__ x, float* __restrict__ part, long long M, int N,
                                                              long long ld, int nsplit) {
    __shared__ float red[4][256];
    const int tid = threadIdx.x, cq = tid & 63, ph = tid >> 6;
    const int col0 = blockIdx.x * 256, col = col0 + cq * 4;
    const long long per = (M + nsplit - 1) / nsplit;
    const long long m0 = blockIdx.y * per, m1 = min(M, m0 + per);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (col + 3 < N) {
        long long m = m0 + ph;
        for (; m + 12 < m1; m += 16) {                                // four independent loads in flight
            const f32x4 a = *reinterpret_cast<const f32x4*>(x + m * ld + col), b = *reinterpret_cast<const f32x4*>(x + (m + 4) * ld + col);
            const f32x4 c = *reinterpret_cast<const f32x4*>(x + (m + 8) * ld + col), e = *reinterpret_cast<const f32x4*>(x + (m + 12) * ld + col);
            acc += a; acc += b; acc += c; acc += e;
        }
        for (; m < m1; m += 4) acc += *reinterpret_cast<const f32x4*>(x + m * ld + col);
    } else {
        for (long long m = m0 + ph; m < m1; m += 4)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (col + e < N) acc[e] += x[m * ld + col + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[ph][cq * 4 + e] = acc[e];
    __syncthreads();
    if (col0 + tid < N) part[(long long)blockIdx.y * N + col0 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ------------------------------------------------------------------ LayerNorm backward (one wave per row)
// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma;  dgamma/dbeta partials per row-block
// R rows of a wave are in flight together (their loads issued back to back, their wave reductions interleaved): with one row at a time the
// four dependent reductions of a row had nothing to overlap with (83 us for 265 MB at the training shape)
template <int MAXV, int R>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ gamma, float* __restrict__ dx,
                                                            float* __restrict__ dgb_part, long long rows, int d, float eps,
                                                            int rows_per_block, const float* __restrict__ res, __bf16* __restrict__ dx16,
                                                            uint32_t drop_thresh, float drop_scale, uint32_t drop_key, long long drop_row0) {
    // Contraction is spelled out (the fused multiply-adds are __builtin_fmaf, everything else rounds operation by operation): left to the
    // compiler, the one-row and the two-row instantiation fused different products of the sums of g and g xhat (ISA of <2, 2> against
    // <2, 1>: the product g = dy gamma contracted into the sum of g, g xhat into its sum, in one float4 slot of one form only), so the two
    // forms that vf_select(VF_SEL_LN_BWD_TWO_ROWS) chooses between differed in the last bits of dx for 256 < d <= 512
#pragma clang fp contract(off)
    // each wave walks rows_per_block/4 rows and keeps per-lane dgamma/dbeta partials in registers
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = d >> 2;
    f32x4 dg[MAXV], db[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) { dg[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; db[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long rend = min(rows, r0 + rows_per_block);
    for (long long rowb = r0 + wave; rowb < rend; rowb += 4 * R) {
        f32x4 xv[R][MAXV], gv[R][MAXV], dyv[R][MAXV];
        long long row[R];
        bool live[R];
        float s[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            live[q] = rowb + 4 * q < rend;
            row[q] = live[q] ? rowb + 4 * q : rowb;             // (a dead slot re-reads the first row and stores nothing)
            s[q] = 0.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int c = lane + 64 * i;
                xv[q][i] = (f32x4){0.f, 0.f, 0.f, 0.f};             // (slots beyond the row stay defined: nothing reads them, but no register
                dyv[q][i] = (f32x4){0.f, 0.f, 0.f, 0.f};            // of this kernel holds an undefined value)
                if (c < nv) {
                    xv[q][i] = *reinterpret_cast<const f32x4*>(x + row[q] * d + c * 4);
                    dyv[q][i] = *reinterpret_cast<const f32x4*>(dy + row[q] * d + c * 4);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
#pragma unroll
            for (int i = 0; i < MAXV; ++i)
                if (lane + 64 * i < nv) s[q] += (xv[q][i][0] + xv[q][i][1]) + (xv[q][i][2] + xv[q][i][3]);
        }
        float mean[R], rstd[R], qq[R], sg[R], sgx[R];
#pragma unroll
        for (int q = 0; q < R; ++q) mean[q] = vf_wave_sum_dpp(s[q]) / (float)d;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            qq[q] = 0.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                if (lane + 64 * i < nv) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float t = xv[q][i][e] - mean[q]; qq[q] += t * t; }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < R; ++q) rstd[q] = 1.0f / sqrtf(vf_wave_sum_dpp(qq[q]) / (float)d + eps);
#pragma unroll
        for (int q = 0; q < R; ++q) {
            sg[q] = 0.f;
            sgx[q] = 0.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int c = lane + 64 * i;
                if (c < nv) {
                    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float xh = (xv[q][i][e] - mean[q]) * rstd[q];
                        const float g = dyv[q][i][e] * gm[e];
                        gv[q][i][e] = g;
                        xv[q][i][e] = xh;
                        sg[q] += g;
                        sgx[q] += g * xh;                           // (product and sum round separately: contraction is off)
                        if (live[q]) {
                            dg[i][e] = __builtin_fmaf(dyv[q][i][e], xh, dg[i][e]);
                            db[i][e] += dyv[q][i][e];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            sg[q] = vf_wave_sum_dpp(sg[q]) / (float)d;
            sgx[q] = vf_wave_sum_dpp(sgx[q]) / (float)d;
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            if (!live[q]) continue;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int c = lane + 64 * i;
                if (c < nv) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = rstd[q] * __builtin_fmaf(-xv[q][i][e], sgx[q], gv[q][i][e] - sg[q]);
                    if (res) {                                      // the residual branch's gradient joins here (was a separate add pass)
                        const f32x4 rv = *reinterpret_cast<const f32x4*>(res + row[q] * d + c * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] += rv[e];
                    }
                    *reinterpret_cast<f32x4*>(dx + row[q] * d + c * 4) = o;
                    if (dx16) {                                     // a bf16 copy for the GEMMs that take this gradient as an operand
                        typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
                        bf16x4_t h;
                        if (drop_thresh) {
                            // the copy's consumer is the backward of a layer whose OUTPUT went through dropout (resid_dropout / the MLP's,
                            // migt.py:216,72): its dY is this gradient under the forward's mask — element (row, col) of mask group
                            // (row >> 2) * d + col, position row & 3 (vf_common.h; the fp32 dx, the residual path's gradient, stays unmasked)
                            const uint32_t g0 = (uint32_t)((row[q] + drop_row0) >> 2) * (uint32_t)d + (uint32_t)(c * 4);
                            const int j = (int)((row[q] + drop_row0) & 3);
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[e] = vf_dropout_keep(vf_dropout_word(drop_key, g0 + e), j, drop_thresh) ? o[e] * drop_scale : 0.f;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) h[e] = (__bf16)o[e];
                        *reinterpret_cast<bf16x4_t*>(dx16 + row[q] * d + c * 4) = h;
                    }
                }
            }
        }
    }
    // the block's four waves combine through LDS in a fixed order, (w0 + w1) + (w2 + w3); partial[block][2][d].  (One slab per WAVE — the first
    // form — made the partial matrix 4800 x 1536 floats at the training shape: 29 MB written and read again per call.)
    __shared__ f32x4 red[3][2][MAXV * 64];
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) { red[wave - 1][0][lane + 64 * i] = dg[i]; red[wave - 1][1][lane + 64 * i] = db[i]; }
    }
    __syncthreads();
    if (wave == 0) {
        float* p = dgb_part + (long long)blockIdx.x * 2 * d;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                f32x4 a, b;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = __fadd_rn(__fadd_rn(dg[i][e], red[0][0][c][e]), __fadd_rn(red[1][0][c][e], red[2][0][c][e]));
                    b[e] = __fadd_rn(__fadd_rn(db[i][e], red[0][1][c][e]), __fadd_rn(red[1][1][c][e], red[2][1][c][e]));
                }
                *reinterpret_cast<f32x4*>(p + c * 4) = a;
                *reinterpret_cast<f32x4*>(p + d + c * 4) = b;
            }
        }
    }
}

// column sums of the [prow][2d] partial matrix straight into dgamma (columns < d) and dbeta: 16 columns per block as four float4 lanes,
// 64 row phases; phases combine by lane shuffles inside a wave and through LDS across the four waves — a fixed order
__global__ __launch_bounds__(256) void layernorm_bwd_final_kernel(const float* __restrict__ part, long long prow, int d, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, int accumulate) {
    __shared__ f32x4 red[4][4];
    const int tid = threadIdx.x, cl = tid & 3, ph = tid >> 2, wave = tid >> 6;
    const int col = blockIdx.x * 16 + cl * 4;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    if (col < 2 * d) {
        long long r = ph;
        for (; r + 64 < prow; r += 128) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(part + r * 2 * d + col);
            const f32x4 b = *reinterpret_cast<const f32x4*>(part + (r + 64) * 2 * d + col);
            s0 += a;
            s1 += b;
        }
        if (r < prow) s0 += *reinterpret_cast<const f32x4*>(part + r * 2 * d + col);
    }
    f32x4 s = s0 + s1;
#pragma unroll
    for (int off = 4; off < 64; off <<= 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += __shfl_xor(s[e], off, 64);
    }
    if ((tid & 63) < 4) red[wave][cl] = s;
    __syncthreads();
    if (tid < 4 && col < 2 * d) {
        const f32x4 t = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
        float* o = col < d ? dgamma + col : dbeta + (col - d);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = accumulate ? o[e] + t[e] : t[e];
    }
}

// ------------------------------------------------------------------ GELU (exact erf) forward / backward
__global__ void gelu_kernel(const float* __restrict__ u, float* __restrict__ f, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        f[i] = vf_gelu_erf(u[i]);
}
__global__ void gelu_bf16out_kernel(const float* __restrict__ u, __bf16* __restrict__ f, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        f[i] = (__bf16)vf_gelu_erf(u[i]);
}
__global__ void gelu_bwd_kernel(const float* __restrict__ u, const float* __restrict__ df, float* __restrict__ du, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        du[i] = __fmul_rn(df[i], vf_gelu_grad(u[i]));
    }
}
__global__ void gelu_bwd_bf16out_kernel(const float* __restrict__ u, const float* __restrict__ df, __bf16* __restrict__ du, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        du[i] = (__bf16)__fmul_rn(df[i], vf_gelu_grad_fast(u[i]));   // the rounding both consumers (dX and dW GEMMs of the bf16 arm) applied on load
    }
}

// ------------------------------------------------------------------ materialised attention softmax with the view mask
__device__ __forceinline__ bool vf_visible(int qv, int kv, int spec) {
    if (spec <= -2) {                       // streams of Sv views (same rule as attention_f32.hip)
        const int Sv = -spec;
        const int qs = qv / Sv, qi = qv - qs * Sv, ks = kv / Sv, ki = kv - ks * Sv;
        return qs == 0 ? (ks == 0 && ki <= qi) : ((ks == 0 && ki < qi) || kv == qv);
    }
    const int Vc = spec >= 0 ? spec : 0x3fffffff;
    return kv == qv || min(kv, Vc) < min(qv, Vc);
}
// one wave per score row: s -> softmax(s*m - 1e4*(1-m)) in place; rows = batch*T, row length T
__global__ __launch_bounds__(256) void softmax_mask_kernel(float* __restrict__ s, long long rows, int T, int L, int spec,
                                                           float scale) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int q = (int)(row % T);
    const int qv = L > 0 ? q / L : 0;
    float* r = s + row * T;
    float mx = -INFINITY;
    for (int c = lane; c < T; c += 64) {
        float v = r[c] * scale;
        if (L > 0 && !vf_visible(qv, c / L, spec)) v = -1e4f;
        r[c] = v;
        mx = fmaxf(mx, v);
    }
    mx = vf_wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < T; c += 64) { const float e = expf(r[c] - mx); r[c] = e; sum += e; }
    sum = vf_wave_sum(sum);
    for (int c = lane; c < T; c += 64) r[c] = r[c] / sum;
}
// dS = P * (dP - sum_j dP*P) * scale, zero where masked (the -1e4 constant and w*0 carry no gradient); in place on dP
__global__ __launch_bounds__(256) void softmax_mask_bwd_kernel(const float* __restrict__ p, float* __restrict__ dp, long long rows,
                                                               int T, int L, int spec, float scale) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int q = (int)(row % T);
    const int qv = L > 0 ? q / L : 0;
    const float* pr = p + row * T;
    float* dr = dp + row * T;
    float dot = 0.f;
    for (int c = lane; c < T; c += 64) dot += pr[c] * dr[c];
    dot = vf_wave_sum(dot);
    for (int c = lane; c < T; c += 64) {
        float g = pr[c] * (dr[c] - dot) * scale;
        if (L > 0 && !vf_visible(qv, c / L, spec)) g = 0.f;
        dr[c] = g;
    }
}

// ------------------------------------------------------------------ softmax cross-entropy (one wave per row)
// loss[r] = lse - logit[target]; dlogits = (softmax - onehot) * w[r]   (sparse_softmax_cross_entropy_with_logits, migt.py:423)
// label smoothing eps (migt.py:99-104): y = onehot (1 - eps) + eps / V  ->  loss = lse - (1 - eps) x[t] - (eps / V) sum_c x[c]
__global__ __launch_bounds__(256) void ce_kernel(const float* __restrict__ logits, const int* __restrict__ target,
                                                 const float* __restrict__ w, float* __restrict__ loss, float* __restrict__ dl,
                                                 long long rows, int V, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = logits + row * V;
    float mx = -INFINITY;
    for (int c = lane; c < V; c += 64) mx = fmaxf(mx, x[c]);
    mx = vf_wave_max(mx);
    float s = 0.f, sx = 0.f;
    for (int c = lane; c < V; c += 64) { s += expf(x[c] - mx); sx += x[c]; }
    s = vf_wave_sum(s);
    const int t = target[row];
    const float lse = mx + logf(s);
    const float uni = eps / (float)V;
    if (eps != 0.f) sx = vf_wave_sum(sx);
    if (lane == 0) loss[row] = eps != 0.f ? lse - (1.f - eps) * x[t] - uni * sx : lse - x[t];
    const float wr = w[row];
    float* d = dl + row * V;
    for (int c = lane; c < V; c += 64) d[c] = (expf(x[c] - mx) / s - ((c == t ? 1.f - eps : 0.f) + uni)) * wr;
}

// ------------------------------------------------------------------ pose MSE (migt.py:156-177): per token
// xyz = raw[0:3] / div[row] (the per-scene random pose multiplier, :160-161; div == nullptr: 1);  y = gt * [pm,pm,pm,1,1,1,1];
// pos = mean_3 (y - xyz)^2 ; ori = mean_4 (y - raw[3:7])^2 ; d raw = 2 (. - y)/k * {w_pos, w_ori}[row] (/ div for xyz)
__global__ void pose_loss_kernel(const float* __restrict__ raw, const float* __restrict__ gt, const float* __restrict__ wp,
                                 const float* __restrict__ wo, const float* __restrict__ div, float* __restrict__ pos,
                                 float* __restrict__ ori, float* __restrict__ draw, long long rows, int L, float pm) {
    const long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float* g = gt + (r / L) * 7;
    const float* x = raw + r * 7;
    float* d = draw + r * 7;
    const float wpr = wp[r], wor = wo[r];
    const float dv = div ? div[r] : 1.f;
    float p = 0.f, o = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float e = x[i] / dv - g[i] * pm; p += e * e; d[i] = 2.f * e / 3.f * wpr / dv; }
#pragma unroll
    for (int i = 3; i < 7; ++i) { const float e = x[i] - g[i]; o += e * e; d[i] = 2.f * e / 4.f * wor; }
    pos[r] = p / 3.f;
    ori[r] = o / 4.f;
}

// ------------------------------------------------------------------ embedding backward (deterministic: no float atomics)
// dwte[id] += sum over the tokens with that id of dh[tok]; dwpe[l] += sum_bs dh[bs][l]; dadd[bs] = sum_l dh[bs][l].
// The first version scattered with float atomicAdd: a third of the training tokens are the MASK id and every position row collects
// B x V terms, so the order of those additions — and the low bits of two whole gradient tensors — changed from run to run (found by
// tests/test_hip_train_full.py; every other reduction of the step was already fixed-order).  Now:
//   embed_bwd_wte_partial: block (id, split s) walks the token range of split s in ascending order and sums its matches -> partial[s][id]
//   embed_bwd_wte_sum:     dwte[id] += partial[0][id] + partial[1][id] + ... in that order
//   embed_bwd_pos:         thread (l, c) walks bs ascending; thread (bs, c) walks l ascending
constexpr int EMB_SPLITS = 16;
constexpr int EMB_U = 8;                                                  // rows in flight per wave
// Round 6: a third of the training tokens carry the MASK id (whole views of the MASK stream), so 16 of the 16 400 blocks did a third of the
// work at four rows per load latency: 256 us for 59 MB.  Now every wave owns a quarter of each 64-token window (its 16 lanes' matches,
// ascending), reads whole rows as float4 (a lane holds columns 4 (lane + 64 j)) with eight rows in flight, and the four wave sums are added
// in wave order — another fixed order than before (results differ in the last bits from round 5's, and are as deterministic).
__global__ __launch_bounds__(256) void embed_bwd_wte_partial_kernel(const float* __restrict__ dh, const int* __restrict__ ids,
                                                                    float* __restrict__ partial, long long ntok, int d, int vocab) {
    extern __shared__ float emb_s[];                                  // [4 waves][d]
    const int id = blockIdx.x, sp = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long per = (ntok + EMB_SPLITS - 1) / EMB_SPLITS;
    const long long t0 = sp * per, t1 = t0 + per < ntok ? t0 + per : ntok;
    const int d4 = d >> 2;                                            // (launcher: d % 4 == 0, d <= 2048)
    float4 acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long base = t0; base < t1; base += 64) {
        int v = -1;
        if (base + lane < t1) {
            v = ids[base + lane];
            v = v < 0 ? 0 : (v >= vocab ? vocab - 1 : v);
        }
        const unsigned long long m = __ballot(v == id);
        unsigned mw = (unsigned)(m >> (16 * wave)) & 0xffffu;           // this wave's quarter of the window
        while (mw) {
            long long tk[EMB_U];
            int n = 0;
#pragma unroll
            for (int u = 0; u < EMB_U; ++u) {
                if (mw) { tk[u] = base + 16 * wave + __builtin_ctz(mw); mw &= mw - 1; n = u + 1; } else tk[u] = base;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c4 = lane + q * 64;
                if (c4 < d4) {
                    float4 x[EMB_U];
#pragma unroll
                    for (int u = 0; u < EMB_U; ++u) x[u] = reinterpret_cast<const float4*>(dh + tk[u] * d)[c4];
#pragma unroll
                    for (int u = 0; u < EMB_U; ++u)
                        if (u < n) { acc[q].x += x[u].x; acc[q].y += x[u].y; acc[q].z += x[u].z; acc[q].w += x[u].w; }   // ascending tokens
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c4 = lane + q * 64;
        if (c4 < d4) reinterpret_cast<float4*>(emb_s + wave * d)[c4] = acc[q];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256)
        partial[((long long)sp * vocab + id) * d + c] = ((emb_s[c] + emb_s[d + c]) + emb_s[2 * d + c]) + emb_s[3 * d + c];
}
// Round 6 (second form): what was left of the kernel above was its SCAN — 16 400 blocks each reading their range's ids (8 rounds of ~19 dependent
// window loads).  With an index built once per token range the row blocks know their rows:
//   embed_bwd_index_kernel  (one block per token range): a stable counting sort in LDS.  The range is cut into T contiguous chunks; integer
//                           atomics count hist[chunk][id] (exact), thread `id` turns its column into chunk offsets, one wave scans the per-id
//                           totals into starts[range][id], and one lane per chunk walks ITS tokens in order, handing out list slots: within
//                           an id the list is in ascending token order whatever the hardware's scheduling
//   embed_bwd_wte_rows_kernel (block (id, range)): the block's rows in four contiguous quarters, one per wave, eight rows in flight, float4;
//                           the four wave sums are added in wave order (a fixed order: deterministic)
// Ranges longer than EMB_MAX_PER tokens, or vocabularies whose histogram does not fit the LDS with at least four chunks, take the scanning kernel above.
constexpr int EMB_MAX_PER = 16384, EMB_IDX_THREADS = 1024, EMB_IDX_LDS = 152 * 1024, EMB_MAX_CHUNKS = 16;
static int embed_index_chunks(long long per, int vocab) {              // chunk owners that fit the LDS budget (0: use the scanning kernel)
    const long long fixed = (per + vocab + 1) * (long long)sizeof(int);
    if (per > EMB_MAX_PER || fixed >= EMB_IDX_LDS) return 0;
    const long long t = (EMB_IDX_LDS - fixed) / ((long long)vocab * (long long)sizeof(int));
    return t >= EMB_MAX_CHUNKS ? EMB_MAX_CHUNKS : (t >= 4 ? (int)t : 0);
}
__global__ __launch_bounds__(EMB_IDX_THREADS) void embed_bwd_index_kernel(const int* __restrict__ ids, int* __restrict__ starts, int* __restrict__ list,
                                                                          long long ntok, int vocab, int nchunk) {
    extern __shared__ int emb_i[];                                    // [per] ids | [vocab + 1] totals -> starts | [nchunk][vocab] counts -> offsets
    const int sp = blockIdx.x, tid = threadIdx.x;
    const long long per = (ntok + EMB_SPLITS - 1) / EMB_SPLITS;
    const long long t0 = sp * per;
    const int n = (int)(t0 >= ntok ? 0 : (t0 + per < ntok ? per : ntok - t0));
    int* sid = emb_i;
    int* tot = emb_i + per;
    int* hist = tot + vocab + 1;
    const int clen = (n + nchunk - 1) / nchunk;                       // tokens per chunk (the last may be short or empty)
    for (int v = tid; v < nchunk * vocab; v += EMB_IDX_THREADS) hist[v] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += EMB_IDX_THREADS) {
        int v = ids[t0 + i];
        v = v < 0 ? 0 : (v >= vocab ? vocab - 1 : v);
        sid[i] = v;
        atomicAdd(&hist[(i / clen) * vocab + v], 1);
    }
    __syncthreads();
    for (int v = tid; v < vocab; v += EMB_IDX_THREADS) {              // counts of an id -> its chunks' offsets within the id; the id's total
        int run = 0;
        for (int t = 0; t < nchunk; ++t) { const int c = hist[t * vocab + v]; hist[t * vocab + v] = run; run += c; }
        tot[v] = run;
    }
    __syncthreads();
    if (tid < 64) {                                                   // exclusive scan of tot[0 .. vocab) by one wave, in place; tot[vocab] = n
        const int chunk = (vocab + 63) / 64;
        const int lo = tid * chunk < vocab ? tid * chunk : vocab, hi = lo + chunk < vocab ? lo + chunk : vocab;
        int sum = 0;
        for (int v = lo; v < hi; ++v) sum += tot[v];
        int incl = sum;                                               // inclusive wave scan of the per-lane sums
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off);
            if (tid >= off) incl += o;
        }
        int run = incl - sum;
        for (int v = lo; v < hi; ++v) { const int c = tot[v]; tot[v] = run; run += c; }
        if (tid == 63) tot[vocab] = n;
    }
    __syncthreads();
    int* st = starts + (long long)sp * (vocab + 1);
    for (int v = tid; v <= vocab; v += EMB_IDX_THREADS) st[v] = tot[v];
    int* ls = list + (long long)sp * EMB_MAX_PER;
    if ((tid & 63) == 0 && (tid >> 6) < nchunk) {                     // one lane per chunk (in its own wave while there are waves)
        for (int t = tid >> 6; t < nchunk; t += EMB_IDX_THREADS / 64) {
            int* h = hist + t * vocab;
            const int i1 = (t + 1) * clen < n ? (t + 1) * clen : n;
            for (int i = t * clen; i < i1; ++i) {
                const int v = sid[i];
                const int k = h[v];
                h[v] = k + 1;
                ls[tot[v] + k] = i;
            }
        }
    }
}

__global__ __launch_bounds__(256) void embed_bwd_wte_rows_kernel(const float* __restrict__ dh, const int* __restrict__ starts,
                                                                 const int* __restrict__ list, float* __restrict__ partial, long long ntok, int d,
                                                                 int vocab) {
    extern __shared__ float emb_s[];                                  // [4 waves][d]
    const int id = blockIdx.x, sp = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int* st = starts + (long long)sp * (vocab + 1);
    const int k0 = st[id], n = st[id + 1] - k0;
    float* out = partial + ((long long)sp * vocab + id) * d;
    if (n == 0) {                                                     // (most (id, range) pairs: nothing to read)
        for (int c = threadIdx.x; c < d; c += 256) out[c] = 0.f;
        return;
    }
    const long long per = (ntok + EMB_SPLITS - 1) / EMB_SPLITS;
    const float* base = dh + (long long)sp * per * d;
    const int* ls = list + (long long)sp * EMB_MAX_PER + k0;
    const int d4 = d >> 2;
    const int q = (n + 3) >> 2;                                       // rows per wave: wave w owns rows [w q, (w + 1) q) of the block's list
    const int r0 = wave * q, r1 = r0 + q < n ? r0 + q : n;
    float4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = r0; r < r1; r += EMB_U) {
        int tk[EMB_U];
#pragma unroll
        for (int u = 0; u < EMB_U; ++u) tk[u] = ls[r + u < r1 ? r + u : r];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c4 = lane + j * 64;
            if (c4 < d4) {
                float4 x[EMB_U];
#pragma unroll
                for (int u = 0; u < EMB_U; ++u) x[u] = reinterpret_cast<const float4*>(base + (long long)tk[u] * d)[c4];
#pragma unroll
                for (int u = 0; u < EMB_U; ++u)
                    if (r + u < r1) { acc[j].x += x[u].x; acc[j].y += x[u].y; acc[j].z += x[u].z; acc[j].w += x[u].w; }
            }
        }
    }
    if (n <= 1) {                                                     // one row: wave 0 holds it
        if (wave == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c4 = lane + j * 64;
                if (c4 < d4) reinterpret_cast<float4*>(out)[c4] = acc[j];
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c4 = lane + j * 64;
        if (c4 < d4) reinterpret_cast<float4*>(emb_s + wave * d)[c4] = acc[j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256) out[c] = ((emb_s[c] + emb_s[d + c]) + emb_s[2 * d + c]) + emb_s[3 * d + c];
}
__global__ void embed_bwd_wte_sum_kernel(const float* __restrict__ partial, float* __restrict__ dwte, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float s = partial[i];
#pragma unroll
        for (int sp = 1; sp < EMB_SPLITS; ++sp) s += partial[sp * n + i];
        dwte[i] += s;
    }
}
__global__ void embed_bwd_pos_kernel(const float* __restrict__ dh, float* __restrict__ dwpe, float* __restrict__ dadd, long long BS,
                                     int L, int d) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long n_pos = (long long)L * d, n_add = BS * d;
    // (eight independent loads in flight, added in ascending order: the sums are the one-load-at-a-time loop's, bit for bit)
    if (i < n_pos) {                                                  // dwpe[l][c]
        float s = 0.f;
        long long bs = 0;
        for (; bs + 8 <= BS; bs += 8) {
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = dh[(bs + u) * n_pos + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += x[u];
        }
        for (; bs < BS; ++bs) s += dh[bs * n_pos + i];
        dwpe[i] += s;
    } else if (i < n_pos + n_add) {                                   // dadd[bs][c]
        const long long j = i - n_pos, bs = j / d, c = j - bs * d;
        const float* p = dh + bs * L * d + c;
        float s = 0.f;
        int l = 0;
        for (; l + 8 <= L; l += 8) {
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = p[(long long)(l + u) * d];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += x[u];
        }
        for (; l < L; ++l) s += p[(long long)l * d];
        dadd[j] = s;
    }
}

// ------------------------------------------------------------------ tiny dense (K <= 16) weight/bias gradient
__global__ void dense_small_k_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dW,
                                         float* __restrict__ db, long long rows, int K, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float acc[16];
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    float b = 0.f;
    for (long long r = 0; r < rows; ++r) {
        const float g = dy[r * N + n];
        b += g;
        for (int k = 0; k < K; ++k) acc[k] = fmaf(x[r * K + k], g, acc[k]);
    }
    for (int k = 0; k < K; ++k) dW[(long long)k * N + n] += acc[k];
    db[n] += b;
}

// one element's step, shared by the per-tensor kernel, the flat kernel and the tile kernel below so that the three agree bit for bit
// (contraction is spelled out: left to the compiler the three kernels fused different products of `b2 v + (1 - b2) g g` — 1-ulp differences in v)
__device__ __forceinline__ void adamw_step(float& w, float gi, float& mi, float& vi, float ld, float lr_adam, float b1, float b2, float eps) {
#pragma clang fp contract(off)
    const float we = __builtin_fmaf(-ld, w, w);
    mi = __builtin_fmaf(b1, mi, (1.f - b1) * gi);
    vi = __builtin_fmaf(b2, vi, ((1.f - b2) * gi) * gi);
    const float q = (lr_adam * mi) / (sqrtf(vi) + eps);
    w = we - q;
}
// ------------------------------------------------------------------ AdamWeightDecay (models/utils.py:507-537 + Keras Adam)
// var -= lr_decay * var (decoupled, before the Adam update); m,v update; var -= lr_adam * m / (sqrt(v) + eps)
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             long long n, float lr_decay, float lr_adam, float b1, float b2, float eps) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float w = p[i], mi = m[i], vi = v[i];
        adamw_step(w, g[i], mi, vi, lr_decay, lr_adam, b1, b2, eps);
        m[i] = mi;
        v[i] = vi;
        p[i] = w;
    }
}

// The whole flat parameter buffer in ONE launch (the per-tensor form above took 468 launches per step): elements inside one of the
// sorted, disjoint [start, end) ranges of `nodecay` (the "bias" tensors, models/utils.py:424) skip the decoupled decay, everything
// else gets it.  Same expressions per element as adamw_kernel (lr_decay = 0 there), so the two forms agree bit for bit.  Tensors start
// on 16-byte boundaries of the flat buffer, so a float4 never straddles two tensors; the padding between them holds zeros.
constexpr int ADAMW_MAX_RANGES = 256;
__device__ __forceinline__ int adamw_first_range_ending_after(const long long* re, int nranges, long long i) {
    int lo = 0, hi = nranges;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (re[mid] > i) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// SKIP: elements inside the (sorted, disjoint) ranges of the pack descriptors belong to adamw_pack_tiles_kernel and are left alone here
template <bool SKIP>
__global__ void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                  long long n4, const long long* __restrict__ nodecay, int nranges, float lr_decay, float lr_adam,
                                  float b1, float b2, float eps, const vf_adamw_pack_desc* __restrict__ descs, int ndesc) {
    __shared__ long long rs[ADAMW_MAX_RANGES], re[ADAMW_MAX_RANGES];
    __shared__ long long ss[SKIP ? ADAMW_MAX_RANGES : 1], se[SKIP ? ADAMW_MAX_RANGES : 1];
    for (int i = threadIdx.x; i < nranges; i += blockDim.x) { rs[i] = nodecay[2 * i]; re[i] = nodecay[2 * i + 1]; }
    if (SKIP)
        for (int i = threadIdx.x; i < ndesc; i += blockDim.x) { ss[i] = descs[i].offset; se[i] = descs[i].offset + (long long)descs[i].rows * descs[i].cols; }
    __syncthreads();
    for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < n4; i4 += (long long)gridDim.x * blockDim.x) {
        const long long i = i4 * 4;
        if (SKIP) {
            const int k = adamw_first_range_ending_after(se, ndesc, i);
            if (k < ndesc && ss[k] <= i) continue;
        }
        const int lo = adamw_first_range_ending_after(re, nranges, i);
        const float ld = (lo < nranges && rs[lo] <= i) ? 0.f : lr_decay;
        f32x4 w = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 gi = *reinterpret_cast<const f32x4*>(g + i);
        f32x4 mi = *reinterpret_cast<const f32x4*>(m + i), vi = *reinterpret_cast<const f32x4*>(v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) { float we = w[e], me = mi[e], ve = vi[e]; adamw_step(we, gi[e], me, ve, ld, lr_adam, b1, b2, eps); w[e] = we; mi[e] = me; vi[e] = ve; }
        *reinterpret_cast<f32x4*>(m + i) = mi;
        *reinterpret_cast<f32x4*>(v + i) = vi;
        *reinterpret_cast<f32x4*>(p + i) = w;
    }
}

// Round 6: the optimizer step and the bf16 re-packing of the dense layers' weights in ONE pass.  The step used to end with adamw_flat (reads w g m v,
// writes w m v) followed by pack_bf16_multi, which read every fp32 weight again TWICE (the [K][N] packing for x @ W and the [N][K] packing for dY @ W^T):
// 0.7 GB of re-reads per step for 88 M weights.  Here a block owns a 16-row x 128-column tile of one weight matrix [rows][cols]: it updates the tile
// (adamw_step: the same expressions, bit-identical parameters and moments), parks the new weights' bf16 roundings in LDS and writes both packings'
// 16-byte groups from there —
//   dst_kn ([K = rows][N = cols] operand, fragment-major [K/64][N/128][ks 4][half 2][n 128][8 k]): the tile is one (k-chunk, ks) x both halves x one
//          128-column block = 256 consecutive groups, 4 KB contiguous;
//   dst_nk ([K = cols][N = rows] operand): 16 column groups x 16 rows, 256-byte runs.
// The layouts are gemm_bf16.hip's (CK = 64, BN = 128); tests/test_train.py compares the result with adamw_flat + pack_bf16_multi bit for bit.
constexpr int AP_ROWS = 16, AP_COLS = 128, AP_LD = AP_COLS + 8, AP_CK = 64, AP_BN = 128;
__global__ __launch_bounds__(256) void adamw_pack_tiles_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                               float lr_decay, float lr_adam, float b1, float b2, float eps,
                                                               const vf_adamw_pack_desc* __restrict__ descs) {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    __shared__ __attribute__((aligned(16))) __bf16 tile[AP_ROWS * AP_LD];
    const vf_adamw_pack_desc d = descs[blockIdx.y];
    if ((d.rows % AP_BN) != 0 || (d.cols % AP_COLS) != 0 || (d.offset & 3)) return;        // (vf_adamw_pack_check refuses such a table on the host)
    const float ld = d.nodecay ? 0.f : lr_decay;                      // (a whole tensor either decays or not; a per-block search of the range table
                                                                      // was eight dependent global loads in front of every tile: 750 us per step)
    const int t = threadIdx.x;
    const int tcols = d.cols / AP_COLS, ntiles = (d.rows / AP_ROWS) * tcols;
    const int nb_kn = d.cols / AP_BN, nb_nk = (d.rows + AP_BN - 1) / AP_BN;
    __bf16* __restrict__ dkn = reinterpret_cast<__bf16*>(d.dst_kn);
    __bf16* __restrict__ dnk = reinterpret_cast<__bf16*>(d.dst_nk);
    for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
        const int tr = ti / tcols, tc = ti - tr * tcols;
        const int r0 = tr * AP_ROWS, c0 = tc * AP_COLS;
        {   // update: thread (row t >> 4, eight columns (t & 15) * 8)
            const int r = t >> 4, c8 = (t & 15) * 8;
            const long long i = d.offset + (long long)(r0 + r) * d.cols + c0 + c8;
            bf16x8_t o;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 w = *reinterpret_cast<const f32x4*>(p + i + 4 * h);
                const f32x4 gi = *reinterpret_cast<const f32x4*>(g + i + 4 * h);
                f32x4 mi = *reinterpret_cast<const f32x4*>(m + i + 4 * h), vi = *reinterpret_cast<const f32x4*>(v + i + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) { float we = w[e], me = mi[e], ve = vi[e]; adamw_step(we, gi[e], me, ve, ld, lr_adam, b1, b2, eps); w[e] = we; mi[e] = me; vi[e] = ve; }
                *reinterpret_cast<f32x4*>(m + i + 4 * h) = mi;
                *reinterpret_cast<f32x4*>(v + i + 4 * h) = vi;
                *reinterpret_cast<f32x4*>(p + i + 4 * h) = w;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[4 * h + e] = (__bf16)w[e];
            }
            *reinterpret_cast<bf16x8_t*>(tile + r * AP_LD + c8) = o;
        }
        __syncthreads();
        if (dkn) {  // [K = rows][N = cols]: group (half = t >> 7, n = t & 127) = rows half * 8 .. + 7 of column n
            const int half = t >> 7, nl = t & 127;
            bf16x8_t o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = tile[(half * 8 + e) * AP_LD + nl];
            const int chunk = r0 / AP_CK, ks = (r0 % AP_CK) >> 4;
            const long long gi = ((((long long)chunk * nb_kn + tc) * 4 + ks) * 2 + half) * AP_BN + nl;
            *reinterpret_cast<bf16x8_t*>(dkn + gi * 8) = o;
        }
        if (dnk) {  // [K = cols][N = rows]: group (eight columns j * 8 .., row rr)
            const int j = t >> 4, rr = t & 15;
            const bf16x8_t o = *reinterpret_cast<const bf16x8_t*>(tile + rr * AP_LD + j * 8);
            const int c = c0 + j * 8, row = r0 + rr;
            const int chunk = c / AP_CK, ks = (c % AP_CK) >> 4, half = (c & 15) >> 3;
            const long long gi = ((((long long)chunk * nb_nk + row / AP_BN) * 4 + ks) * 2 + half) * AP_BN + (row % AP_BN);
            *reinterpret_cast<bf16x8_t*>(dnk + gi * 8) = o;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dropout: out = x * keep / (1 - rate) [+ res]
// x [rows][cols] row-major; element (m, n) belongs to mask group (m >> 2) * cols + n at position m & 3 (vf_common.h)
__global__ void dropout_add_kernel(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ out,
                                   long long rows, int cols, long long row0, uint32_t thresh, float scale, uint32_t seed, uint32_t site) {
    const long long n = rows * cols;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / cols;
        const uint32_t c = (uint32_t)(i - m * cols);
        const float v = vf_dropout_keep_elem(seed, site, (uint64_t)(m + row0), c, (uint32_t)cols, thresh) ? x[i] * scale : 0.f;
        out[i] = res ? v + res[i] : v;
    }
}
// cols % 4 == 0, 16-byte aligned pointers: one float4 per thread (four columns of one row: four mask groups)
__global__ void dropout_add4_kernel(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ out,
                                    long long rows, int cols, long long row0, uint32_t thresh, float scale, uint32_t seed, uint32_t site) {
    const int c4 = cols >> 2;
    const long long n4 = rows * c4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / c4;
        const uint32_t c = (uint32_t)(i - m * c4) * 4u;
        const uint64_t g = ((uint64_t)(m + row0) >> 2) * (uint64_t)cols + c;
        const int j = (int)((m + row0) & 3);
        f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t ge = g + e;
            const uint32_t w = vf_dropout_word(vf_dropout_key(seed, site, (uint32_t)(ge >> 32)), (uint32_t)ge);
            v[e] = vf_dropout_keep(w, j, thresh) ? v[e] * scale : 0.f;
        }
        if (res) {
            const f32x4 r = *reinterpret_cast<const f32x4*>(res + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += r[e];
        }
        *reinterpret_cast<f32x4*>(out + 4 * i) = v;
    }
}

// ------------------------------------------------------------------ axpy-style helpers
__global__ void add_inplace_kernel(float* __restrict__ a, const float* __restrict__ b, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) a[i] += b[i];
}
__global__ void axpby_kernel(float a, const float* __restrict__ x, float b, const float* __restrict__ y, float* __restrict__ out,
                             long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = a * x[i] + (y ? b * y[i] : 0.f);
}
// Global sum of squares without a float atomic (the rule of the embedding backward below holds here too: the clip factor scales every
// gradient, so its low bits must not depend on scheduling).  Block b of at most CLIP_MAX_PARTIALS writes part[b]: its threads' strided
// sums folded by the fixed butterfly of vf_wave_sum, the four wave sums added in wave order.  Every block of the scaling kernel then
// adds the partials in one fixed order of its own (clip_total), so all blocks hold the same bits and no further launch is needed.
constexpr int CLIP_MAX_PARTIALS = 1024;
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, float* __restrict__ part, long long n) {
    __shared__ float red[4];
    float s = 0.f;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) s += x[i] * x[i];
    s = vf_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
// thread t adds part[4 t .. 4 t + 3] in index order; the 256 sums are folded as in sumsq_kernel (256-thread blocks only)
__device__ __forceinline__ float clip_total(const float* __restrict__ part, int nparts) {
    __shared__ float red[4];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CLIP_MAX_PARTIALS / 256; ++j) {
        const int k = (int)threadIdx.x * (CLIP_MAX_PARTIALS / 256) + j;
        if (k < nparts) s += part[k];
    }
    s = vf_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, const float* __restrict__ part, int nparts, float clip, long long n) {
    // tf.clip_by_norm: x * clip / max(norm, clip)
    const float norm = sqrtf(clip_total(part, nparts));
    const float f = clip / fmaxf(norm, clip);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) x[i] *= f;
}
__global__ __launch_bounds__(256) void scale_gradnorm_kernel(float* __restrict__ x, const float* __restrict__ part, int nparts, float max_norm,
                                                             long long n) {
    // torch.nn.utils.clip_grad_norm_: coef = max_norm / (total_norm + 1e-6); grads *= coef only when coef < 1
    const float f = max_norm / (sqrtf(clip_total(part, nparts)) + 1e-6f);
    if (!(f < 1.0f)) return;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) x[i] *= f;
}


// ---- tiny-N dense layer and its weight gradient (round 6): the pose head's c_proj is 1536 -> 7 (migt.py:291-292,354; QuaternionPoseRepresentation).  On the
// implicit-GEMM kernel (N padded to a 32-column tile, 50 workgroups for 6 400 rows) the forward and the dW = X^T dY each took 176 us of a 20 ms training
// step — for 0.14 GFLOP and 39 MB.  Both are one pass over X at HBM rate:
//   forward: one wave per row, lanes stride the K axis in float4 steps, W^T staged in LDS [n][K], N <= 8 accumulators per lane, DPP wave sums;
//   dW: a workgroup owns a slab of rows and every k (threads stride K), dY's row is a broadcast, N <= 8 accumulators per owned k; slab partials
//       are folded by vf_sum_slabs_f32 in slab order (deterministic).
constexpr int SN_MAX = 8;
__global__ __launch_bounds__(256) void dense_small_n_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
                                                            float* __restrict__ out, long long rows, int K, int N, long long ldx) {
    extern __shared__ __attribute__((aligned(16))) float wt[];          // [SN_MAX][K]: W transposed (zero rows beyond N)
    for (int i = threadIdx.x; i < SN_MAX * K; i += 256) {
        const int n = i / K, k = i - n * K;
        wt[i] = n < N ? W[(size_t)k * N + n] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k4 = K >> 2;
    for (long long r = (long long)blockIdx.x * 4 + wave; r < rows; r += (long long)gridDim.x * 4) {
        const f32x4* __restrict__ xr = reinterpret_cast<const f32x4*>(x + r * ldx);
        float acc[SN_MAX];
#pragma unroll
        for (int n = 0; n < SN_MAX; ++n) acc[n] = 0.f;
        for (int c = lane; c < k4; c += 64) {
            const f32x4 xv = xr[c];
#pragma unroll
            for (int n = 0; n < SN_MAX; ++n) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + n * K + 4 * c);
                acc[n] = __builtin_fmaf(xv[0], wv[0], __builtin_fmaf(xv[1], wv[1], __builtin_fmaf(xv[2], wv[2], __builtin_fmaf(xv[3], wv[3], acc[n]))));
            }
        }
#pragma unroll
        for (int n = 0; n < SN_MAX; ++n) acc[n] = vf_wave_sum_dpp(acc[n]);
        if (lane == 0) {
            for (int n = 0; n < N; ++n) out[r * N + n] = acc[n] + (b ? b[n] : 0.f);
        }
    }
}

// slab[blockIdx.x][k][n] = sum over the slab's rows of x[m][k] * dy[m][n]; thread t owns k = t, t + 256, ...
template <int KPT>
__global__ __launch_bounds__(256) void dense_small_n_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ slabs,
                                                                  long long rows, int K, int N, long long ldx, int rows_per_slab) {
    __shared__ float dys[64][SN_MAX];
    const long long m0 = (long long)blockIdx.x * rows_per_slab;
    const long long m1 = m0 + rows_per_slab < rows ? m0 + rows_per_slab : rows;
    float acc[KPT][SN_MAX];
#pragma unroll
    for (int i = 0; i < KPT; ++i)
#pragma unroll
        for (int n = 0; n < SN_MAX; ++n) acc[i][n] = 0.f;
    for (long long mb = m0; mb < m1; mb += 64) {
        const int nr = (int)(m1 - mb < 64 ? m1 - mb : 64);
        __syncthreads();
        for (int i = threadIdx.x; i < 64 * SN_MAX; i += 256) {
            const int r = i / SN_MAX, n = i - r * SN_MAX;
            dys[r][n] = (r < nr && n < N) ? dy[(mb + r) * N + n] : 0.f;
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const float* __restrict__ xr = x + (mb + r) * ldx;
            float xv[KPT];
#pragma unroll
            for (int i = 0; i < KPT; ++i) { const int k = threadIdx.x + 256 * i; xv[i] = k < K ? xr[k] : 0.f; }
#pragma unroll
            for (int n = 0; n < SN_MAX; ++n) {
                const float d = dys[r][n];
#pragma unroll
                for (int i = 0; i < KPT; ++i) acc[i][n] = __builtin_fmaf(xv[i], d, acc[i][n]);
            }
        }
    }
    float* __restrict__ o = slabs + (size_t)blockIdx.x * K * N;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + 256 * i;
        if (k < K)
            for (int n = 0; n < N; ++n) o[(size_t)k * N + n] = acc[i][n];
    }
}

}  // namespace

extern "C" {

int vf_transpose_f32(const float* src, float* dst, int rows, int cols, int64_t ld_src, int64_t ld_dst, int batch,
                     int64_t bs_src, int64_t bs_dst, void* stream) {
    if (!src || !dst || rows <= 0 || cols <= 0 || batch < 1 || ld_src < cols || ld_dst < rows) return VF_ERR_BAD_ARG;
    dim3 grid((cols + 31) / 32, (rows + 31) / 32, batch);
    hipLaunchKernelGGL(transpose_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, rows, cols, (long long)ld_src,
                       (long long)ld_dst, (long long)bs_src, (long long)bs_dst);
    return vf_last_status();
}

int vf_transpose_bf16_f32(const void* src_bf16, float* dst, int rows, int cols, int64_t ld_src, int64_t ld_dst, int batch,
                          int64_t bs_src, int64_t bs_dst, void* stream) {
    if (!src_bf16 || !dst || rows <= 0 || cols <= 0 || batch < 1 || ld_src < cols || ld_dst < rows) return VF_ERR_BAD_ARG;
    dim3 grid((cols + 31) / 32, (rows + 31) / 32, batch);
    hipLaunchKernelGGL(transpose_kernel<__bf16>, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const __bf16*>(src_bf16), dst,
                       rows, cols, (long long)ld_src, (long long)ld_dst, (long long)bs_src, (long long)bs_dst);
    return vf_last_status();
}

size_t vf_colsum_workspace_bytes(int N) { return N > 0 ? (size_t)256 * N * sizeof(float) : 0; }

// rows per split 128, at most max_split splits (= rows of the [split][N] scratch the caller provides): the bias gradients of
// the training step reduce 19200 x 768..3072 matrices, which 64 splits x 3..12 column blocks left on a fraction of the CUs
static int colsum_launch(const float* x, float* out, int64_t M, int N, int64_t ld, int accumulate, void* ws, int max_split,
                         void* stream) {
    if (!x || !out || !ws || M <= 0 || N <= 0 || ld < N) return VF_ERR_BAD_ARG;
    int nsplit = (int)((M + 127) / 128);
    if (nsplit > max_split) nsplit = max_split;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((N + 255) / 256, nsplit), dim3(256), 0, s, x, (float*)ws, (long long)M, N,
                       (long long)ld, nsplit);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const float*)ws, out, N, nsplit, accumulate);
    return vf_last_status();
}

int vf_colsum_f32(const float* x, float* out, int64_t M, int N, int64_t ld, int accumulate, void* ws, void* stream) {
    if (!x || !out || !ws || M <= 0 || N <= 0 || ld < N) return VF_ERR_BAD_ARG;
    if ((ld & 3) || ((uintptr_t)x & 15) || N < 64) return colsum_launch(x, out, M, N, ld, accumulate, ws, 256, stream);   // narrow / unaligned: one column per thread
    int nsplit = (int)((M + 127) / 128);
    if (nsplit > 256) nsplit = 256;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(colsum_partial4_kernel, dim3((N + 255) / 256, nsplit), dim3(256), 0, s, x, (float*)ws, (long long)M, N, (long long)ld, nsplit);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const float*)ws, out, N, nsplit, accumulate);
    return vf_last_status();
}

// rows per block of the backward kernel (4 per wave).  64 rows per block left the 19 200-row training matrices on 1200 waves — about one
// per SIMD, each walking 16 rows whose four dependent wave reductions nothing overlapped: 76-105 us for 236 MB (2.2 TB/s).  Round 3, at
// 19 200 x 768 with the residual and the bf16 copy (265 MB), kernel + finalize: 16 rows, one row at a time, four float4 slots per lane 89 us;
// three slots (d = 768 exactly) 69-70 us; two rows in flight 62-64 us (4.2-4.3 TB/s; the shipped form, see the launcher for its history);
// 8 rows per block 64-65, 4 rows 70-80; wave sums by DPP adds instead of ds_bpermute: 67.5 / 61.2 us (tools/bench_ln_bwd.py)
constexpr int LN_BWD_RPB = 16;
size_t vf_layernorm_bwd_workspace_bytes(int64_t rows, int d) {
    if (rows <= 0 || d <= 0) return 0;
    const int64_t blocks = (rows + LN_BWD_RPB - 1) / LN_BWD_RPB;
    return (size_t)blocks * 2 * d * sizeof(float);      // [blocks][2d] per-block partials of dgamma | dbeta
}

int vf_layernorm_bwd_f32(const float* dy, const float* x, const float* gamma, float* dx, float* dgamma, float* dbeta,
                         int64_t rows, int d, float eps, int accumulate, const float* res, void* dx_bf16, float drop_rate, uint32_t drop_seed,
                         uint32_t drop_site, int64_t drop_row0, void* ws, void* stream) {
    if (!dy || !x || !gamma || !dx || !dgamma || !dbeta || !ws || rows <= 0 || d <= 0) return VF_ERR_BAD_ARG;
    if ((d & 3) || d > 1024) return VF_ERR_UNSUPPORTED;
    if (!(drop_rate >= 0.f && drop_rate < 1.f) || (drop_rate > 0.f && !dx_bf16) || drop_row0 < 0) return VF_ERR_BAD_ARG;
    if (drop_rate > 0.f && (unsigned long long)((rows + drop_row0 + 3) / 4) * (unsigned long long)d >= (1ull << 32)) return VF_ERR_UNSUPPORTED;   // 32-bit mask groups
    const uint32_t dthr = vf_dropout_thresh(drop_rate), dkey = vf_dropout_key(drop_seed, drop_site, 0u);
    const float dscale = 1.0f / (1.0f - drop_rate);
    const int rpb = LN_BWD_RPB;
    const unsigned blocks = (unsigned)((rows + rpb - 1) / rpb);
    hipStream_t s = (hipStream_t)stream;
    __bf16* d16 = reinterpret_cast<__bf16*>(dx_bf16);
    // Two rows of a wave in flight (62 us against 68-70 for one row at the training shape; vf_select(VF_SEL_LN_BWD_TWO_ROWS, 0) selects the one-row form, same bits: the kernel spells its contraction out,
    // tests/test_hip_transformer_kernels.py compares the two forms at every width).
    // History of this switch (round 3): with the wave sums on ds_bpermute (vf_wave_sum) the two-row form was bit-identical in a process that
    // owns the GPU but NOT bit-reproducible when a second process shared the device — the 2-rank gloo test on one GPU failed every other
    // run; tools/flaky_probe2.py traced it to ~1 call in 75 returning a few rows of dx ~1e-4 off on identical inputs (0 of 6 000 calls with
    // the one-row form).  With the sums on DPP adds (vf_wave_sum_dpp) both forms are reproducible there (0 of 5 000 calls): two interleaved
    // ds_bpermute chains do not survive the context switches of a shared GPU; nothing else in the library interleaves them.
    const bool one = !vf_selected(VF_SEL_LN_BWD_TWO_ROWS);
#define VF_LN_BWD_LAUNCH(MV, RR) hipLaunchKernelGGL((layernorm_bwd_kernel<MV, RR>), dim3(blocks), dim3(256), 0, s, dy, x, gamma, dx, (float*)ws, \
                                                    (long long)rows, d, eps, rpb, res, d16, dthr, dscale, dkey, (long long)drop_row0)
    if (d <= 256) { if (one) VF_LN_BWD_LAUNCH(1, 1); else VF_LN_BWD_LAUNCH(1, 2); }
    else if (d <= 512) { if (one) VF_LN_BWD_LAUNCH(2, 1); else VF_LN_BWD_LAUNCH(2, 2); }
    else if (d <= 768) { if (one) VF_LN_BWD_LAUNCH(3, 1); else VF_LN_BWD_LAUNCH(3, 2); }      // (d_model 768: three float4 per lane exactly)
    else { if (one) VF_LN_BWD_LAUNCH(4, 1); else VF_LN_BWD_LAUNCH(4, 2); }
#undef VF_LN_BWD_LAUNCH
    int st = vf_last_status();
    if (st) return st;
    hipLaunchKernelGGL(layernorm_bwd_final_kernel, dim3((unsigned)((2 * d + 15) / 16)), dim3(256), 0, s, (const float*)ws, (long long)blocks, d, dgamma,
                       dbeta, accumulate);
    return vf_last_status();
}

int vf_gelu_bwd_bf16out_f32(const float* u, const float* df, void* du_bf16, int64_t n, void* stream) {
    if (!u || !df || !du_bf16 || n < 0) return VF_ERR_BAD_ARG;
    if (n == 0) return VF_OK;
    hipLaunchKernelGGL(gelu_bwd_bf16out_kernel, dim3(grid1(n, 256)), dim3(256), 0, (hipStream_t)stream, u, df, reinterpret_cast<__bf16*>(du_bf16),
                       (long long)n);
    return vf_last_status();
}

int vf_gelu_f32(const float* u, float* f, int64_t n, void* stream) {
    if (!u || !f || n < 0) return VF_ERR_BAD_ARG;
    if (n == 0) return VF_OK;
    hipLaunchKernelGGL(gelu_kernel, dim3(grid1(n, 256)), dim3(256), 0, (hipStream_t)stream, u, f, (long long)n);
    return vf_last_status();
}

int vf_gelu_bf16out_f32(const float* u, void* f_bf16, int64_t n, void* stream) {
    if (!u || !f_bf16 || n < 0) return VF_ERR_BAD_ARG;
    if (n == 0) return VF_OK;
    hipLaunchKernelGGL(gelu_bf16out_kernel, dim3(grid1(n, 256)), dim3(256), 0, (hipStream_t)stream, u, reinterpret_cast<__bf16*>(f_bf16), (long long)n);
    return vf_last_status();
}

int vf_gelu_bwd_f32(const float* u, const float* df, float* du, int64_t n, void* stream) {
    if (!u || !df || !du || n < 0) return VF_ERR_BAD_ARG;
    if (n == 0) return VF_OK;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(grid1(n, 256)), dim3(256), 0, (hipStream_t)stream, u, df, du, (long long)n);
    return vf_last_status();
}

int vf_softmax_mask_f32(float* s, int64_t batch, int T, int L, int mask_spec, float scale, void* stream) {
    if (!s || batch <= 0 || T <= 0 || L < 0) return VF_ERR_BAD_ARG;
    const long long rows = (long long)batch * T;
    hipLaunchKernelGGL(softmax_mask_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s, rows, T, L,
                       mask_spec, scale);
    return vf_last_status();
}

int vf_softmax_mask_bwd_f32(const float* p, float* dp, int64_t batch, int T, int L, int mask_spec, float scale, void* stream) {
    if (!p || !dp || batch <= 0 || T <= 0 || L < 0) return VF_ERR_BAD_ARG;
    const long long rows = (long long)batch * T;
    hipLaunchKernelGGL(softmax_mask_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, dp, rows,
                       T, L, mask_spec, scale);
    return vf_last_status();
}

int vf_softmax_ce_f32(const float* logits, const int32_t* target, const float* row_weight, float* loss, float* dlogits,
                      int64_t rows, int V, float label_smoothing, void* stream) {
    if (!logits || !target || !row_weight || !loss || !dlogits || rows <= 0 || V <= 0) return VF_ERR_BAD_ARG;
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return VF_ERR_BAD_ARG;
    hipLaunchKernelGGL(ce_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, target, row_weight,
                       loss, dlogits, (long long)rows, V, label_smoothing);
    return vf_last_status();
}

int vf_pose_mse_f32(const float* raw, const float* gt, const float* w_pos, const float* w_ori, const float* xyz_div, float* pos_loss,
                    float* ori_loss, float* draw, int64_t rows, int L, float position_multiplier, void* stream) {
    if (!raw || !gt || !w_pos || !w_ori || !pos_loss || !ori_loss || !draw || rows <= 0 || L <= 0) return VF_ERR_BAD_ARG;
    hipLaunchKernelGGL(pose_loss_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, raw, gt, w_pos,
                       w_ori, xyz_div, pos_loss, ori_loss, draw, (long long)rows, L, position_multiplier);
    return vf_last_status();
}

size_t vf_embed_bwd_workspace_bytes(int d, int vocab) {
    if (d <= 0 || vocab <= 0) return 0;
    // partial sums [ranges][vocab][d] | starts [ranges][vocab + 1] | row lists [ranges][EMB_MAX_PER]
    return (size_t)EMB_SPLITS * vocab * d * sizeof(float) + (size_t)EMB_SPLITS * ((size_t)vocab + 1 + EMB_MAX_PER) * sizeof(int);
}

int vf_embed_bwd_f32(const float* dh, const int32_t* ids, float* dwte, float* dwpe, float* dadd, int64_t BS, int L, int d,
                     int vocab, void* workspace, void* stream) {
    if (!dh || !ids || !dwte || !dwpe || !dadd || !workspace || BS <= 0 || L <= 0 || d <= 0 || vocab <= 0) return VF_ERR_BAD_ARG;
    if (d > 2048 || d % 4 != 0 || (reinterpret_cast<uintptr_t>(dh) & 15) != 0) return VF_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    float* partial = reinterpret_cast<float*>(workspace);
    const long long ntok = (long long)BS * L, per = (ntok + EMB_SPLITS - 1) / EMB_SPLITS;
    const int nchunk = embed_index_chunks(per, vocab);
    if (nchunk) {
        int* starts = reinterpret_cast<int*>(partial + (size_t)EMB_SPLITS * vocab * d);
        int* list = starts + (size_t)EMB_SPLITS * (vocab + 1);
        const size_t smem = ((size_t)per + vocab + 1 + (size_t)nchunk * vocab) * sizeof(int);
        static unsigned long long attr_devs = 0;
        if (vf_attr_needed(&attr_devs)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(embed_bwd_index_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, EMB_IDX_LDS);
            if (e != hipSuccess) return (int)e;
            vf_attr_done(&attr_devs);
        }
        hipLaunchKernelGGL(embed_bwd_index_kernel, dim3(EMB_SPLITS), dim3(EMB_IDX_THREADS), smem, s, ids, starts, list, ntok, vocab, nchunk);
        hipLaunchKernelGGL(embed_bwd_wte_rows_kernel, dim3((unsigned)vocab, EMB_SPLITS), dim3(256), (size_t)4 * d * sizeof(float), s, dh, starts, list, partial,
                           ntok, d, vocab);
    } else {
        hipLaunchKernelGGL(embed_bwd_wte_partial_kernel, dim3((unsigned)vocab, EMB_SPLITS), dim3(256), (size_t)4 * d * sizeof(float), s, dh, ids, partial,
                           ntok, d, vocab);
    }
    const long long n = (long long)vocab * d;
    hipLaunchKernelGGL(embed_bwd_wte_sum_kernel, dim3(grid1(n, 256, 4096)), dim3(256), 0, s, partial, dwte, n);
    const long long m = (long long)L * d + (long long)BS * d;
    hipLaunchKernelGGL(embed_bwd_pos_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, dh, dwpe, dadd, (long long)BS, L, d);
    return vf_last_status();
}

int vf_dense_small_k_bwd_f32(const float* x, const float* dy, float* dW, float* db, int64_t rows, int K, int N, void* stream) {
    if (!x || !dy || !dW || !db || rows <= 0 || K <= 0 || N <= 0) return VF_ERR_BAD_ARG;
    if (K > 16) return VF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dense_small_k_bwd_kernel, dim3((N + 127) / 128), dim3(128), 0, (hipStream_t)stream, x, dy, dW, db,
                       (long long)rows, K, N);
    return vf_last_status();
}

int vf_adamw_f32(float* param, const float* grad, float* m, float* v, int64_t n, float lr_decay, float lr_adam, float beta1,
                 float beta2, float eps, void* stream) {
    if (!param || !grad || !m || !v || n < 0) return VF_ERR_BAD_ARG;
    if (n == 0) return VF_OK;
    hipLaunchKernelGGL(adamw_kernel, dim3(grid1(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, param, grad, m, v, (long long)n,
                       lr_decay, lr_adam, beta1, beta2, eps);
    return vf_last_status();
}

int vf_adamw_flat_f32(float* param, const float* grad, float* m, float* v, int64_t n, const int64_t* nodecay_ranges, int nranges,
                      float lr_decay, float lr_adam, float beta1, float beta2, float eps, void* stream) {
    if (!param || !grad || !m || !v || n < 0 || nranges < 0 || (nranges > 0 && !nodecay_ranges)) return VF_ERR_BAD_ARG;
    if ((n & 3) || nranges > ADAMW_MAX_RANGES || (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15)) return VF_ERR_UNSUPPORTED;
    if (n == 0) return VF_OK;
    hipLaunchKernelGGL(adamw_flat_kernel<false>, dim3(grid1(n / 4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, param, grad, m, v,
                       (long long)(n / 4), reinterpret_cast<const long long*>(nodecay_ranges), nranges, lr_decay, lr_adam, beta1, beta2, eps,
                       (const vf_adamw_pack_desc*)nullptr, 0);
    return vf_last_status();
}

size_t vf_sizeof_adamw_pack_desc(void) { return sizeof(vf_adamw_pack_desc); }

int vf_adamw_pack_check(const vf_adamw_pack_desc* descs_host, int ndesc, int64_t n) {
    if (!descs_host || ndesc <= 0 || n < 0) return VF_ERR_BAD_ARG;
    if (ndesc > ADAMW_MAX_RANGES) return VF_ERR_UNSUPPORTED;
    int64_t prev_end = 0;
    for (int i = 0; i < ndesc; ++i) {
        const vf_adamw_pack_desc& d = descs_host[i];
        if (d.rows <= 0 || d.cols <= 0 || d.offset < prev_end || (!d.dst_kn && !d.dst_nk)) return VF_ERR_BAD_ARG;      // sorted, disjoint
        if ((d.rows % AP_BN) || (d.cols % AP_COLS) || (d.offset & 3)) return VF_ERR_UNSUPPORTED;      // (whole 128-blocks both ways: the packings have no padding to zero)
        if (((uintptr_t)d.dst_kn | (uintptr_t)d.dst_nk) & 15) return VF_ERR_UNSUPPORTED;
        prev_end = d.offset + (int64_t)d.rows * d.cols;
        if (prev_end > n) return VF_ERR_BAD_ARG;
    }
    return VF_OK;
}

int vf_adamw_flat_pack_f32(float* param, const float* grad, float* m, float* v, int64_t n, const int64_t* nodecay_ranges, int nranges,
                           float lr_decay, float lr_adam, float beta1, float beta2, float eps, const vf_adamw_pack_desc* descs_device, int ndesc,
                           void* stream) {
    if (!param || !grad || !m || !v || n < 0 || nranges < 0 || (nranges > 0 && !nodecay_ranges) || !descs_device || ndesc <= 0) return VF_ERR_BAD_ARG;
    if ((n & 3) || nranges > ADAMW_MAX_RANGES || ndesc > ADAMW_MAX_RANGES || (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15))
        return VF_ERR_UNSUPPORTED;
    if (n == 0) return VF_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adamw_pack_tiles_kernel, dim3(1024, (unsigned)ndesc), dim3(256), 0, s, param, grad, m, v, lr_decay, lr_adam, beta1, beta2, eps,
                       descs_device);
    hipLaunchKernelGGL(adamw_flat_kernel<true>, dim3(grid1(n / 4, 256, 8192)), dim3(256), 0, s, param, grad, m, v, (long long)(n / 4),
                       reinterpret_cast<const long long*>(nodecay_ranges), nranges, lr_decay, lr_adam, beta1, beta2, eps, descs_device, ndesc);
    return vf_last_status();
}

int vf_add_inplace_f32(float* a, const float* b, int64_t n, void* stream) {
    if (!a || !b || n < 0) return VF_ERR_BAD_ARG;
    if (n == 0) return VF_OK;
    hipLaunchKernelGGL(add_inplace_kernel, dim3(grid1(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, a, b, (long long)n);
    return vf_last_status();
}

int vf_dropout_add_f32(const float* x, const float* res, float* out, int64_t rows, int cols, int64_t row0, float rate, uint32_t seed,
                       uint32_t site, void* stream) {
    if (!x || !out || rows < 0 || cols <= 0 || row0 < 0 || !(rate >= 0.f && rate < 1.f)) return VF_ERR_BAD_ARG;
    if (rows == 0) return VF_OK;
    const uint32_t thresh = vf_dropout_thresh(rate);
    const float scale = 1.0f / (1.0f - rate);
    const long long n = (long long)rows * cols;
    if ((cols & 3) == 0 && !(((uintptr_t)x | (uintptr_t)out | (uintptr_t)res) & 15))
        hipLaunchKernelGGL(dropout_add4_kernel, dim3(grid1(n / 4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, res, out, (long long)rows, cols,
                           (long long)row0, thresh, scale, seed, site);
    else
        hipLaunchKernelGGL(dropout_add_kernel, dim3(grid1(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, res, out, (long long)rows, cols,
                           (long long)row0, thresh, scale, seed, site);
    return vf_last_status();
}

int vf_axpby_f32(float a, const float* x, float b, const float* y, float* out, int64_t n, void* stream) {
    if (!x || !out || n < 0) return VF_ERR_BAD_ARG;
    if (n == 0) return VF_OK;
    hipLaunchKernelGGL(axpby_kernel, dim3(grid1(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, a, x, b, y, out, (long long)n);
    return vf_last_status();
}

/* floats of scratch the two clip entry points need (the per-block partial sums of squares) */
int vf_clip_scratch_floats(void) { return CLIP_MAX_PARTIALS; }

int vf_clip_by_norm_f32(float* x, int64_t n, float clip, float* scratch, void* stream) {
    if (!x || !scratch || n <= 0 || clip <= 0.f) return VF_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nparts = grid1(n, 256, CLIP_MAX_PARTIALS);
    hipLaunchKernelGGL(sumsq_kernel, dim3(nparts), dim3(256), 0, s, x, scratch, (long long)n);
    hipLaunchKernelGGL(scale_kernel, dim3(grid1(n, 256, 8192)), dim3(256), 0, s, x, scratch, (int)nparts, clip, (long long)n);
    return vf_last_status();
}

int vf_clip_grad_norm_f32(float* x, int64_t n, float max_norm, float* scratch, void* stream) {
    if (!x || !scratch || n <= 0 || !(max_norm > 0.f)) return VF_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nparts = grid1(n, 256, CLIP_MAX_PARTIALS);
    hipLaunchKernelGGL(sumsq_kernel, dim3(nparts), dim3(256), 0, s, x, scratch, (long long)n);
    hipLaunchKernelGGL(scale_gradnorm_kernel, dim3(grid1(n, 256, 8192)), dim3(256), 0, s, x, scratch, (int)nparts, max_norm, (long long)n);
    return vf_last_status();
}


/* out[r][n] = sum_k x[r][k] W[k][n] + b[n] for a tiny N (<= 8; the pose head's 1536 -> 7): one pass over x at HBM rate.  K % 4 == 0, K <= 4096,
 * ldx % 4 == 0, 16-byte aligned x */
int vf_dense_small_n_f32(const float* x, const float* W, const float* b, float* out, int64_t rows, int K, int N, int64_t ldx, void* stream) {
    if (!x || !W || !out || rows < 0 || K <= 0 || N <= 0 || ldx < K) return VF_ERR_BAD_ARG;
    if (N > SN_MAX || (K & 3) || K > 4096 || (ldx & 3) || (reinterpret_cast<uintptr_t>(x) & 15)) return VF_ERR_UNSUPPORTED;
    if (rows == 0) return VF_OK;
    const size_t smem = (size_t)SN_MAX * K * sizeof(float);
    static unsigned long long attr_devs = 0;
    if (smem > 64 * 1024 && vf_attr_needed(&attr_devs)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dense_small_n_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (e != hipSuccess) return (int)e;
        vf_attr_done(&attr_devs);
    }
    const long long wgs = (rows + 3) / 4;
    hipLaunchKernelGGL(dense_small_n_kernel, dim3((unsigned)(wgs < 1024 ? wgs : 1024)), dim3(256), smem, (hipStream_t)stream, x, W, b, out, (long long)rows, K,
                       N, (long long)ldx);
    return vf_last_status();
}

/* number of slabs (and the rows per slab) vf_dense_small_n_wgrad_f32 writes for `rows` rows: the caller provides slabs * K * N floats of workspace */
int vf_dense_small_n_wgrad_slabs(int64_t rows) {
    if (rows <= 0) return 0;
    const long long per = rows >= 256 * 32 ? 32 : 16;                 /* >= 200 workgroups at the step's 6 400 rows */
    return (int)((rows + per - 1) / per);
}

/* dW[k][n] (+)= sum_r x[r][k] dy[r][n] for a tiny N (<= 8), K <= 2048: slab partial sums (workspace), folded in slab order */
int vf_dense_small_n_wgrad_f32(const float* x, const float* dy, float* dW, float* ws, int64_t rows, int K, int N, int64_t ldx, int accumulate,
                               void* stream) {
    if (!x || !dy || !dW || !ws || rows <= 0 || K <= 0 || N <= 0 || ldx < K) return VF_ERR_BAD_ARG;
    if (N > SN_MAX || K > 2048) return VF_ERR_UNSUPPORTED;
    const int slabs = vf_dense_small_n_wgrad_slabs(rows);
    const int per = (int)((rows + slabs - 1) / slabs);
    hipStream_t s = (hipStream_t)stream;
    const int kpt = (K + 255) / 256;
    if (kpt <= 2) hipLaunchKernelGGL(dense_small_n_wgrad_kernel<2>, dim3(slabs), dim3(256), 0, s, x, dy, ws, (long long)rows, K, N, (long long)ldx, per);
    else if (kpt <= 4) hipLaunchKernelGGL(dense_small_n_wgrad_kernel<4>, dim3(slabs), dim3(256), 0, s, x, dy, ws, (long long)rows, K, N, (long long)ldx, per);
    else hipLaunchKernelGGL(dense_small_n_wgrad_kernel<8>, dim3(slabs), dim3(256), 0, s, x, dy, ws, (long long)rows, K, N, (long long)ldx, per);
    if (int st = vf_last_status()) return st;
    return vf_sum_slabs_f32(ws, slabs, (int64_t)K * N, (int64_t)K * N, dW, accumulate, stream);
}

}  // extern "C"
