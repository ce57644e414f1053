// Prefix-cache attention of the novel-view renderer, gfx950: N independent QUERY views per scene, each attending to the scene's C cached
// context views (the "prefix": C*L keys whose K / V were computed once by MIGT.prefill_context) plus the L keys of its own view, and to
// nothing else.  That is the visibility of a twin view under vf_attn_blockcausal_*'s twin mask (an "alternative ending" of the sequence),
// for any number of endings, with the prefix read from where the prefill left it instead of being recomputed per ending.
//
// No mask logic: every key a query walks is visible to it, and the keys it does not walk are the ones whose "w*m - 1e4*(1-m)" weight is an
// exact fp32 zero (what skip_masked exploits in the block-causal kernels).  Scores are un-scaled (branching_attention.py:7), softmax fp32.
//
// Work layout: a workgroup serves a GROUP of consecutive query views of one (scene, head) — four in the bf16 arm (a wave = the 64 queries of
// one view, as attention_lp.hip), two in the fp32-equivalent arm (a wave = 32 queries, as attention_x6.hip) — and stages every prefix K / V
// tile into LDS ONCE for the whole group; then the group's own tiles go through the same LDS buffers one after the other, each consumed by
// the waves of its view only.  A wave's arithmetic depends on its own view and the prefix alone, never on which views share its group: a
// query's result is bit-identical whatever N, whatever the position of the view in the launch.  Keys are walked in ascending order, prefix
// first, own view last — the order of the twin-mask pass — with the arithmetic of attention_lp.hip (bf16 arm: the same bits as its
// register-staged kernel) and of attention_x6.hip (fp32-equivalent arm: the same bits).
//
// Variable context lengths (vf_attn_prefix_var_*, the kernels' VAR instantiation): a length per query view, ctx_len[b*N + n] in [0, C]
// (clamped on read; C is the cache's capacity).  The layout above stays: the group walks gmax = the longest length among its own views, so
// each prefix tile is still staged once; a wave consumes prefix tile s only if s < its own length and otherwise only helps staging; own
// tiles follow at steps gmax, gmax + 1, ...  A group whose lengths are all 0 starts with an own tile.  A wave without a view (last partial
// group) counts as length 0 and reads no length.  Contract:
//   - a view with length c >= 1 gets, bit for bit, what the fixed-C entry gives it with C = c on the same buffers and prefix_stride,
//     whatever the other views' lengths, N, or its position: its key order (prefix ascending, then own) and arithmetic are the same;
//   - the kernel writes exactly the logical output elements;
//   - a view's result does not depend on cache rows at or beyond its length.
// The fixed-C instantiation compiles to what it was (gmax = mylen = C are the same value): same bits, same registers.
//
// Forked caches (vf_attn_prefix_fork_*, the kernels' FORK instantiation): the logical context of child scene b is the first split[b] views of
// PARENT scene b / share (kp / vp, read where they lie) followed by the scene's OWN views (kp2 / vp2, addressed by b).  Lengths count logical
// views and work as in VAR; split is clamped to [0, C] and a length to [0, split + C2] on read, so no value of either array takes a load
// outside either buffer (own view s - split < C2 whenever it is read; with C2 = 0 the own segment is never read).  All views of a workgroup
// belong to one scene, so the segment of step s — and with it the base pointer, leading dimension and view number in prefetch(s) — is uniform
// in the workgroup.  Staging, the group logic, the key order (parent ascending, own ascending, the view's own tile) and the arithmetic are
// those of VAR: a view gets the bits that VAR gives it on the materialised cache (parent views [0, split) and the own views, contiguous).
// The fixed-C and VAR instantiations take prefix_args as before and compile to what they were.
//
// Packed caches (vf_attn_prefix_q8_bf16, the bf16 kernel's Q8 instantiation; csrc/kv_pack.hip makes them): the prefix is e4m3 bytes in
// 64 x 64 tiles — K [key][feature], V [feature][key], the transposed image the V^T LDS rows want — with one power-of-two fp32 scale per
// (scene, view, head).  Only prefetch and stage differ from VAR: a prefix step fetches each tile as one contiguous 4 KiB block (16 bytes per
// thread) and its scale by a load that is uniform in the workgroup; stage converts, multiplies by the scale and casts to bf16 — exact,
// since an e4m3 value times a power of two is a bf16 number — and writes the LDS image the other modes build (K rows as 16-byte writes,
// V^T rows, 136 B apart, as 8-byte writes).  The group's own tiles come from q / k / v as before.  The consumer half of the loop, the key
// order, gmax / mylen, the softmax and the stores are shared: a view gets, bit for bit, what VAR gives it on the dequantised cache.  A
// length is clamped to [0, C], so no value of ctx_len takes a load outside the packed buffers.  FIXED, VAR and FORK compile to what they were.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int DH = 64;
constexpr int LV = 64;      // tokens per view = keys per tile
constexpr int GV16 = 4;     // query views per workgroup, bf16 arm
constexpr int GV32 = 2;     // query views per workgroup, fp32-equivalent arm

struct prefix_args {
    const void* q; const void* k; const void* v;      // query views' thirds of the fused c_attn output, rows [B*N*L]
    const void* kp; const void* vp;                   // prefix K / V, rows [C*L] per scene, scenes pstride elements apart
    void* out;
    int C, N;
    int ldq, ldk, ldv, ldkp, ldvp, ldo;
    long long pstride;
    int in16, out16;
    const int* ctx_len;                               // VAR / FORK: [B*N] context lengths, one per query view
};

// FORK: the second (own) segment and the mapping; B counts CHILD scenes
struct fork_args : prefix_args {
    const void* kp2; const void* vp2;                 // own K / V, rows [C2*L] per child scene, scenes pstride2 elements apart
    int C2, share;                                    // room of the own segment in views; child scene b reads parent scene b / share
    int ldkp2, ldvp2;
    long long pstride2;
    const int* split;                                 // [B]: logical view s of scene b is parent view s if s < split[b], else own view s - split[b]
};

// Q8 (bf16 arm only): the prefix is a PACKED cache (csrc/kv_pack.hip) — e4m3 tiles with one power-of-two scale each; kp / vp are not read
struct q8_args : prefix_args {
    const unsigned char* kq; const unsigned char* vq;  // tile (b, s, h) at b * qscene + s * qview + h * 4096 bytes: K [key][feature], V [feature][key]
    const float* kscale; const float* vscale;          // its scales at b * sscene + s * sview + h
    long long qview, qscene, sview, sscene;
};

enum { FIXED = 0, VAR = 1, FORK = 2, Q8 = 3 };
template <int MODE> struct args_of { typedef prefix_args type; };
template <> struct args_of<FORK> { typedef fork_args type; };
template <> struct args_of<Q8> { typedef q8_args type; };

// VAR / FORK: the length of query view (b, n), clamped to the room (VAR: the cache's capacity; FORK: the scene's split + the own room); fixed-C: C
template <int MODE>
__device__ __forceinline__ int view_len(const prefix_args& a, size_t b, int n, int room) {
    if constexpr (MODE != FIXED) return min(max(a.ctx_len[b * (size_t)a.N + (size_t)n], 0), room);
    else return a.C;
}

__device__ __forceinline__ f32x4 load4(const void* base, size_t off, int in16) {
    if (in16) {
        const bf16x4 t = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(base) + off);
        return f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
    }
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + off);
}

// ------------------------------------------------------------------------------------------------------------------- bf16 arm
constexpr int K_LDB = 144;            // K row [key][dh] bf16: 128 B + 16 (conflict-free ds_read_b128)
constexpr int VT_LDB = 136;           // V^T row [feature][key] bf16: 128 B + 8

template <int MODE>
__global__ __launch_bounds__(256, 2) void attn_prefix_bf16_kernel(const typename args_of<MODE>::type a) {
    __shared__ __attribute__((aligned(16))) unsigned char Ks[LV * K_LDB];
    __shared__ __attribute__((aligned(16))) unsigned char Vt[DH * VT_LDB];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const int h = blockIdx.x;
    const size_t b = blockIdx.y;
    const int v0 = (int)blockIdx.z * GV16;                       // the group's first query view
    const int nown = min(GV16, a.N - v0);                        // views of this group (>= 1)
    const bool active = wave < nown;                             // this wave has a view (otherwise it only helps moving tiles)
    const size_t qrow0 = (b * (size_t)a.N + (size_t)(v0 + (active ? wave : 0))) * LV;     // first row of this wave's view
    const int in16 = a.in16;

    // ---- Q fragments (B operand of S^T = K.Q^T): qb[u][ks] = Q[32 u + l31][16 ks + 8 half + 0..7]
    bf16x8 qb[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const size_t ro = (qrow0 + 32 * u + l31) * (size_t)a.ldq + h * DH + 8 * half;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const f32x4 t0 = load4(a.q, ro + 16 * ks, in16), t1 = load4(a.q, ro + 16 * ks + 4, in16);
#pragma unroll
            for (int e = 0; e < 4; ++e) { qb[u][ks][e] = (__bf16)t0[e]; qb[u][ks][4 + e] = (__bf16)t1[e]; }
        }
    }

    // staging map: thread -> 4-feature column tid&15; K rows (tid>>4) + 16 i; V key pairs 2p, 2p+1 with p = (tid>>4) + 16 (i>>1)
    const int s_col4 = tid & 15;
    const int s_row0 = tid >> 4;
    // VAR: the wave walks its own view's first mylen prefix tiles; the group stages gmax = its longest member's (a wave without a view
    // counts as length 0 and reads no length)
    int mylen = a.C, gmax = a.C;
    int split = a.C;                                             // FORK: the scene's first own view (parent views below it), uniform in the workgroup
    size_t pscene = b;                                           // the scene of the kp / vp segment
    if constexpr (MODE != FIXED) {
        int room = a.C;
        if constexpr (MODE == FORK) {
            split = min(max(a.split[b], 0), a.C);
            room = split + a.C2;
            pscene = b / (size_t)a.share;
        }
        gmax = 0;
        for (int j = 0; j < nown; ++j) gmax = max(gmax, view_len<MODE>(a, b, v0 + j, room));
        mylen = active ? view_len<MODE>(a, b, v0 + wave, room) : 0;
    }
    const int nsteps = gmax + nown;                              // gmax prefix tiles, then the group's own tiles
    f32x4 kreg[4], vreg[4];
    uint4 kq8, vq8;                                              // Q8: this thread's 16 bytes of the packed K tile and of the packed V^T tile
    float ksc = 0.f, vsc = 0.f;                                  //     and the tile's two scales (uniform in the workgroup)
    auto prefetch = [&](int s) {
        if constexpr (MODE == Q8) {
            if (s < gmax) {                                          // a prefix tile: one contiguous 4 KiB block each for K and V^T
                const size_t t0 = b * (size_t)a.qscene + (size_t)s * (size_t)a.qview + (size_t)h * (LV * DH) + (size_t)tid * 16;
                kq8 = *reinterpret_cast<const uint4*>(a.kq + t0);
                vq8 = *reinterpret_cast<const uint4*>(a.vq + t0);
                const size_t s0 = b * (size_t)a.sscene + (size_t)s * (size_t)a.sview + (size_t)h;
                ksc = a.kscale[s0];
                vsc = a.vscale[s0];
                return;
            }
        }
        const void *kb, *vb;
        size_t k0, v0_;
        int ldk_, ldv_;
        bool own2 = false;
        if constexpr (MODE == FORK) own2 = s >= split && s < gmax;
        if (own2) {
            if constexpr (MODE == FORK) {                            // own view s - split < C2 of child scene b
                kb = a.kp2; vb = a.vp2; ldk_ = a.ldkp2; ldv_ = a.ldvp2;
                k0 = b * (size_t)a.pstride2 + (size_t)(s - split) * LV * ldk_ + h * DH;
                v0_ = b * (size_t)a.pstride2 + (size_t)(s - split) * LV * ldv_ + h * DH;
            }
        } else if (s < gmax) {
            kb = a.kp; vb = a.vp; ldk_ = a.ldkp; ldv_ = a.ldvp;
            k0 = pscene * (size_t)a.pstride + (size_t)s * LV * ldk_ + h * DH;
            v0_ = pscene * (size_t)a.pstride + (size_t)s * LV * ldv_ + h * DH;
        } else {
            kb = a.k; vb = a.v; ldk_ = a.ldk; ldv_ = a.ldv;
            const size_t r0 = (b * (size_t)a.N + (size_t)(v0 + s - gmax)) * LV;
            k0 = r0 * ldk_ + h * DH;
            v0_ = r0 * ldv_ + h * DH;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = s_row0 + 16 * i;
            const int vkey = 2 * (s_row0 + 16 * (i >> 1)) + (i & 1);
            kreg[i] = load4(kb, k0 + (size_t)key * ldk_ + s_col4 * 4, in16);
            vreg[i] = load4(vb, v0_ + (size_t)vkey * ldv_ + s_col4 * 4, in16);
        }
    };
    auto stage = [&](int s) {
        if constexpr (MODE == Q8) {
            if (s < gmax) {                                          // e4m3 * 2^e is a bf16 value: the LDS image is the one VAR builds from the unpacked cache
                const int r = tid >> 2, c16 = tid & 3;               // K: key r, features 16 c16 ...; V^T: feature r, keys 16 c16 ...
                bf16x8 k8[2];
                bf16x4 v4[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned kw = w == 0 ? kq8.x : w == 1 ? kq8.y : w == 2 ? kq8.z : kq8.w;
                    const unsigned vw = w == 0 ? vq8.x : w == 1 ? vq8.y : w == 2 ? vq8.z : vq8.w;
                    const auto k01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)kw, false), k23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)kw, true);
                    const auto v01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vw, false), v23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vw, true);
                    k8[w >> 1][4 * (w & 1) + 0] = (__bf16)(k01[0] * ksc);
                    k8[w >> 1][4 * (w & 1) + 1] = (__bf16)(k01[1] * ksc);
                    k8[w >> 1][4 * (w & 1) + 2] = (__bf16)(k23[0] * ksc);
                    k8[w >> 1][4 * (w & 1) + 3] = (__bf16)(k23[1] * ksc);
                    v4[w][0] = (__bf16)(v01[0] * vsc);
                    v4[w][1] = (__bf16)(v01[1] * vsc);
                    v4[w][2] = (__bf16)(v23[0] * vsc);
                    v4[w][3] = (__bf16)(v23[1] * vsc);
                }
                *reinterpret_cast<bf16x8*>(Ks + r * K_LDB + c16 * 32) = k8[0];
                *reinterpret_cast<bf16x8*>(Ks + r * K_LDB + c16 * 32 + 16) = k8[1];
#pragma unroll
                for (int w = 0; w < 4; ++w) *reinterpret_cast<bf16x4*>(Vt + r * VT_LDB + c16 * 32 + 8 * w) = v4[w];   // rows of 136 B: 8-byte aligned
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf16x4 kk;
#pragma unroll
            for (int e = 0; e < 4; ++e) kk[e] = (__bf16)kreg[i][e];
            *reinterpret_cast<bf16x4*>(Ks + (s_row0 + 16 * i) * K_LDB + s_col4 * 8) = kk;
        }
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
            const int p2 = 2 * (s_row0 + 16 * ip);                   // even key of the pair
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bf16x2 pr;
                pr[0] = (__bf16)vreg[2 * ip][e];
                pr[1] = (__bf16)vreg[2 * ip + 1][e];
                *reinterpret_cast<bf16x2*>(Vt + (s_col4 * 4 + e) * VT_LDB + p2 * 2) = pr;
            }
        }
    };

    f32x16 ot[2][2];                                                 // [query tile][feature half]
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[u][d][r] = 0.f;
    float m_run[2] = {-INFINITY, -INFINITY};
    float l_run[2] = {0.f, 0.f};
    constexpr float LOG2E = 1.4426950408889634f;

    prefetch(0);
    for (int s = 0; s < nsteps; ++s) {
        __syncthreads();                                             // previous tile fully consumed
        stage(s);
        __syncthreads();
        if (s + 1 < nsteps) prefetch(s + 1);
        if (!active || (s >= gmax ? s - gmax != wave : s >= mylen)) continue;      // an own tile belongs to one wave; a prefix tile to the views that reach it

        // ---- S^T = K . Q^T: each K fragment (LDS) feeds both query tiles
        f32x16 st[2][2];                                             // [query tile][key half]
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[u][t2][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (t2 * 32 + l31) * K_LDB + (ks * 16 + half * 8) * 2);
#pragma unroll
                for (int u = 0; u < 2; ++u) st[u][t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qb[u][ks], st[u][t2], 0, 0, 0);
            }

        // ---- online softmax (lane = one query of each tile; its 32 keys of this key tile)
        bf16x8 pb[2][2][2];                                          // [query tile][key half][k-step]
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float mx = -INFINITY;
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                for (int r = 0; r < 16; r += 2) mx = __builtin_fmaxf(__builtin_fmaxf(mx, st[u][t2][r]), st[u][t2][r + 1]);   // v_max3_f32
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run[u], mx);
            const float alpha = __builtin_amdgcn_exp2f((m_run[u] - m_new) * LOG2E);       // 0 on the first tile (m_run = -inf)
            const float mc = m_new * LOG2E;
            float psum = 0.f;
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[u][t2][ks2 * 8 + e], LOG2E, -mc));
                        psum += p;
                        pb[u][t2][ks2][e] = (__bf16)p;
                    }
            l_run[u] = l_run[u] * alpha + psum;
            m_run[u] = m_new;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {        // the maximum moved for some query of the wave: rescale
#pragma unroll
                for (int d = 0; d < 2; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) ot[u][d][r] *= alpha;
            }
        }

        // ---- O^T += V^T . P^T: k-step (t2, ks2) = keys 32 t2 + 16 ks2 + 8 (e>>2) + 4 half + (e&3); each V^T fragment feeds both tiles
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const unsigned char* vrow = Vt + (d * 32 + l31) * VT_LDB + (t2 * 32 + 16 * ks2 + 4 * half) * 2;
                    const bf16x4 va0 = *reinterpret_cast<const bf16x4*>(vrow);
                    const bf16x4 va1 = *reinterpret_cast<const bf16x4*>(vrow + 16);
                    bf16x8 va;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { va[e] = va0[e]; va[4 + e] = va1[e]; }
#pragma unroll
                    for (int u = 0; u < 2; ++u) ot[u][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb[u][t2][ks2], ot[u][d], 0, 0, 0);
                }
    }

    // ---- normalise and store: lane = query, regs 4j..4j+3 = 4 consecutive features
    if (!active) return;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const float l_tot = l_run[u] + __shfl_xor(l_run[u], 32, 64);
        const size_t oo = (qrow0 + 32 * u + l31) * (size_t)a.ldo + h * DH + 4 * half;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = ot[u][d][4 * j + e] / l_tot;
                if (a.out16) {                                       // bf16 output for a bf16-MFMA consumer (ldo in elements)
                    bf16x4 o4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o4[e] = (__bf16)o[e];
                    *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(a.out) + oo + d * 32 + 8 * j) = o4;
                } else {
                    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + oo + d * 32 + 8 * j) = o;
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------- fp32-equivalent arm (x6)
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)x;
    const float r1 = x - (float)h;
    m = (__bf16)r1;
    l = (__bf16)(r1 - (float)m);
}

constexpr int K6_LDB = 400;   // bytes per K row in LDS: 3 planes x 128 B + 16 B pad (attention_x6.hip)
constexpr int VT6_LDB = 392;  // bytes per V^T row: 3 planes x 128 B + 8 B pad

template <int MODE>
__global__ __launch_bounds__(256, 2) void attn_prefix_x6_kernel(const typename args_of<MODE>::type a) {
    __shared__ __attribute__((aligned(16))) unsigned char Ks[LV * K6_LDB];
    __shared__ __attribute__((aligned(16))) unsigned char Vt[DH * VT6_LDB];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const int h = blockIdx.x;
    const size_t b = blockIdx.y;
    const int v0 = (int)blockIdx.z * GV32;
    const int nown = min(GV32, a.N - v0);
    const int slot = wave >> 1;                                  // the wave's view of the group: two waves of 32 queries per view
    const bool active = slot < nown;
    const size_t qrow = (b * (size_t)a.N + (size_t)(v0 + (active ? slot : 0))) * LV + (wave & 1) * 32 + l31;

    const float* qf = reinterpret_cast<const float*>(a.q);
    float* of = reinterpret_cast<float*>(a.out);

    // ---- Q fragment (B operand): qb[plane][ks][e] = piece of Q[qrow][16 ks + 8 half + e]
    bf16x8 qb[3][4];
    {
        const float* src = qf + qrow * (size_t)a.ldq + h * DH + 8 * half;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(src + 16 * ks);
            const f32x4 t1 = *reinterpret_cast<const f32x4*>(src + 16 * ks + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                __bf16 hh, mm, ll;
                split3(e < 4 ? t0[e & 3] : t1[e & 3], hh, mm, ll);
                qb[0][ks][e] = hh; qb[1][ks][e] = mm; qb[2][ks][e] = ll;
            }
        }
    }

    const int s_col4 = tid & 15;
    const int s_row0 = tid >> 4;
    int mylen = a.C, gmax = a.C;                                 // as the bf16 arm
    int split = a.C;
    size_t pscene = b;
    if constexpr (MODE != FIXED) {
        int room = a.C;
        if constexpr (MODE == FORK) {
            split = min(max(a.split[b], 0), a.C);
            room = split + a.C2;
            pscene = b / (size_t)a.share;
        }
        gmax = 0;
        for (int j = 0; j < nown; ++j) gmax = max(gmax, view_len<MODE>(a, b, v0 + j, room));
        mylen = active ? view_len<MODE>(a, b, v0 + slot, room) : 0;
    }
    const int nsteps = gmax + nown;
    f32x4 kreg[4], vreg[4];
    auto prefetch = [&](int s) {
        const float *kb, *vb;
        int ldk_, ldv_;
        bool own2 = false;
        if constexpr (MODE == FORK) own2 = s >= split && s < gmax;
        if (own2) {
            if constexpr (MODE == FORK) {                            // own view s - split < C2 of child scene b
                ldk_ = a.ldkp2; ldv_ = a.ldvp2;
                kb = reinterpret_cast<const float*>(a.kp2) + b * (size_t)a.pstride2 + (size_t)(s - split) * LV * ldk_ + h * DH;
                vb = reinterpret_cast<const float*>(a.vp2) + b * (size_t)a.pstride2 + (size_t)(s - split) * LV * ldv_ + h * DH;
            }
        } else if (s < gmax) {
            ldk_ = a.ldkp; ldv_ = a.ldvp;
            kb = reinterpret_cast<const float*>(a.kp) + pscene * (size_t)a.pstride + (size_t)s * LV * ldk_ + h * DH;
            vb = reinterpret_cast<const float*>(a.vp) + pscene * (size_t)a.pstride + (size_t)s * LV * ldv_ + h * DH;
        } else {
            ldk_ = a.ldk; ldv_ = a.ldv;
            const size_t r0 = (b * (size_t)a.N + (size_t)(v0 + s - gmax)) * LV;
            kb = reinterpret_cast<const float*>(a.k) + r0 * ldk_ + h * DH;
            vb = reinterpret_cast<const float*>(a.v) + r0 * ldv_ + h * DH;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = s_row0 + 16 * i;
            const int vkey = 2 * (s_row0 + 16 * (i >> 1)) + (i & 1);
            kreg[i] = *reinterpret_cast<const f32x4*>(kb + (size_t)key * ldk_ + s_col4 * 4);
            vreg[i] = *reinterpret_cast<const f32x4*>(vb + (size_t)vkey * ldv_ + s_col4 * 4);
        }
    };

    f32x16 ot[2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[d][r] = 0.f;
    float m_run = -INFINITY;
    float l_run = 0.f;

    prefetch(0);
    for (int s = 0; s < nsteps; ++s) {
        __syncthreads();   // previous tile fully consumed
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf16x4 kh, km, kl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                __bf16 hh, mm, ll;
                split3(kreg[i][e], hh, mm, ll);
                kh[e] = hh; km[e] = mm; kl[e] = ll;
            }
            unsigned char* dst = Ks + (s_row0 + 16 * i) * K6_LDB + s_col4 * 8;
            *reinterpret_cast<bf16x4*>(dst) = kh;
            *reinterpret_cast<bf16x4*>(dst + 128) = km;
            *reinterpret_cast<bf16x4*>(dst + 256) = kl;
        }
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
            const int p2 = 2 * (s_row0 + 16 * ip);                   // even key of the pair
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bf16x2 ph, pm, pl;
                __bf16 hh, mm, ll;
                split3(vreg[2 * ip][e], hh, mm, ll);
                ph[0] = hh; pm[0] = mm; pl[0] = ll;
                split3(vreg[2 * ip + 1][e], hh, mm, ll);
                ph[1] = hh; pm[1] = mm; pl[1] = ll;
                unsigned char* dst = Vt + (s_col4 * 4 + e) * VT6_LDB + p2 * 2;
                *reinterpret_cast<bf16x2*>(dst) = ph;
                *reinterpret_cast<bf16x2*>(dst + 128) = pm;
                *reinterpret_cast<bf16x2*>(dst + 256) = pl;
            }
        }
        __syncthreads();
        if (s + 1 < nsteps) prefetch(s + 1);
        if (!active || (s >= gmax ? s - gmax != slot : s >= mylen)) continue;      // an own tile belongs to the two waves of its view

        // ---- S^T = K . Q^T
        f32x16 st[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[t2][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                bf16x8 ka[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    ka[pl] = *reinterpret_cast<const bf16x8*>(Ks + (t2 * 32 + l31) * K6_LDB + pl * 128 + ks * 32 + half * 16);
                constexpr int PA[6] = {2, 0, 1, 1, 0, 0};      // plane 0 = h, 1 = m, 2 = l; smallest products first
                constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
                for (int t = 0; t < 6; ++t)
                    st[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[PA[t]], qb[PB[t]][ks], st[t2], 0, 0, 0);
            }
        }

        // ---- online softmax (lane = one query; its 32 keys of this tile)
        float mx = -INFINITY;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[t2][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        constexpr float LOG2E = 1.4426950408889634f;
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);   // 0 on the first tile (m_run = -inf)
        float psum = 0.f;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f((st[t2][r] - m_new) * LOG2E);
                st[t2][r] = p;
                psum += p;
            }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[d][r] *= alpha;

        // ---- O^T += V^T . P^T
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int ks2 = 0; ks2 < 2; ++ks2) {
                bf16x8 pb[3];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    __bf16 hh, mm, ll;
                    split3(st[t2][ks2 * 8 + e], hh, mm, ll);
                    pb[0][e] = hh; pb[1][e] = mm; pb[2][e] = ll;
                }
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const unsigned char* vrow = Vt + (d * 32 + l31) * VT6_LDB + (t2 * 32 + 16 * ks2 + 4 * half) * 2;
                    bf16x8 va[3];
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) {
                        const bf16x4 w0 = *reinterpret_cast<const bf16x4*>(vrow + pl * 128);
                        const bf16x4 w1 = *reinterpret_cast<const bf16x4*>(vrow + pl * 128 + 16);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { va[pl][e] = w0[e]; va[pl][4 + e] = w1[e]; }
                    }
                    constexpr int PA[6] = {2, 0, 1, 1, 0, 0};
                    constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
                    for (int t = 0; t < 6; ++t)
                        ot[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va[PA[t]], pb[PB[t]], ot[d], 0, 0, 0);
                }
            }
    }

    // ---- normalise and store: lane = query, regs 4j..4j+3 = 4 consecutive features
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (active) {
        float* orow = of + qrow * (size_t)a.ldo + h * DH + 4 * half;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = ot[d][4 * j + e] / l_tot;
                *reinterpret_cast<f32x4*>(orow + d * 32 + 8 * j) = o;
            }
    }
}

// arguments every arm checks before it launches anything (host only: no device needed)
int prefix_check(const prefix_args& a, int B, int H, int L, int dh) {
    if (B < 0 || a.N < 0 || H <= 0 || a.C < 0) return VF_ERR_BAD_ARG;
    if (!a.q || !a.k || !a.v || !a.kp || !a.vp || !a.out) return VF_ERR_BAD_ARG;
    if (L != LV || dh != DH || a.C < 1) return VF_ERR_UNSUPPORTED;
    if (a.ldq < H * DH || a.ldk < H * DH || a.ldv < H * DH || a.ldkp < H * DH || a.ldvp < H * DH || a.ldo < H * DH) return VF_ERR_BAD_ARG;
    const long long al = a.in16 ? 7 : 3;                         // rows are read as 8- / 16-byte vectors
    if (((long long)(a.ldq | a.ldk | a.ldv | a.ldkp | a.ldvp) | a.pstride) & al) return VF_ERR_BAD_ARG;
    if (a.ldo & 3) return VF_ERR_BAD_ARG;
    if (a.pstride < 0) return VF_ERR_BAD_ARG;
    if (B > 65535 || H > 65535 || a.N > 2 * 65535) return VF_ERR_UNSUPPORTED;       // grid dimensions y / x / z
    return VF_OK;
}

// the own segment and the mapping of a fork (host only); B = 0 / N = 0 are no-ops AFTER these checks, as everywhere
int fork_check(const fork_args& a, int H) {
    if (!a.split || a.share < 1 || a.C2 < 0) return VF_ERR_BAD_ARG;
    if (a.C2 > 0 && (!a.kp2 || !a.vp2)) return VF_ERR_BAD_ARG;   // C2 = 0: the own segment is never read, its pointers may be NULL
    if (a.ldkp2 < H * DH || a.ldvp2 < H * DH) return VF_ERR_BAD_ARG;
    const long long al = a.in16 ? 7 : 3;
    if (((long long)(a.ldkp2 | a.ldvp2) | a.pstride2) & al) return VF_ERR_BAD_ARG;
    if (a.pstride2 < 0) return VF_ERR_BAD_ARG;
    return VF_OK;
}

// the packed prefix (host only)
int q8_check(const q8_args& a, int B, int H) {
    if (!a.kq || !a.vq || !a.kscale || !a.vscale) return VF_ERR_BAD_ARG;
    if (((uintptr_t)a.kq | (uintptr_t)a.vq) & 15 || ((uintptr_t)a.kscale | (uintptr_t)a.vscale) & 3) return VF_ERR_BAD_ARG;
    if (a.qview < (long long)H * LV * DH || a.qscene < 0 || (a.qview | a.qscene) & 15) return VF_ERR_BAD_ARG;   // tiles are fetched as 16-byte vectors
    if (a.sview < H || a.sscene < 0) return VF_ERR_BAD_ARG;
    return VF_OK;
}

template <int MODE>
int launch_bf16(const typename args_of<MODE>::type& a, int B, int H, int L, int dh, void* stream) {
    if (MODE != FIXED && !a.ctx_len) return VF_ERR_BAD_ARG;
    int rc = prefix_check(a, B, H, L, dh);
    if constexpr (MODE == FORK) {
        if (rc == VF_OK) rc = fork_check(a, H);
    }
    if constexpr (MODE == Q8) {
        if (rc == VF_OK) rc = q8_check(a, B, H);
    }
    if (rc != VF_OK) return rc;
    if (B == 0 || a.N == 0) return VF_OK;
    dim3 grid((unsigned)H, (unsigned)B, (unsigned)((a.N + GV16 - 1) / GV16));
    hipLaunchKernelGGL(attn_prefix_bf16_kernel<MODE>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return vf_last_status();
}

template <int MODE>
int launch_x6(const typename args_of<MODE>::type& a, int B, int H, int L, int dh, void* stream) {
    if (MODE != FIXED && !a.ctx_len) return VF_ERR_BAD_ARG;
    int rc = prefix_check(a, B, H, L, dh);
    if constexpr (MODE == FORK) {
        if (rc == VF_OK) rc = fork_check(a, H);
    }
    if (rc != VF_OK) return rc;
    if (B == 0 || a.N == 0) return VF_OK;
    dim3 grid((unsigned)H, (unsigned)B, (unsigned)((a.N + GV32 - 1) / GV32));
    hipLaunchKernelGGL(attn_prefix_x6_kernel<MODE>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return vf_last_status();
}

}  // namespace

extern "C" {

int vf_attn_prefix_bf16(const void* q, const void* k, const void* v, const void* kp, const void* vp, int in_bf16, void* out, int out_bf16,
                        int B, int H, int C, int N, int L, int dh, int ldq, int ldk, int ldv, int ldkp, int ldvp, int64_t prefix_stride,
                        int ldo, void* stream) {
    const prefix_args a{q, k, v, kp, vp, out, C, N, ldq, ldk, ldv, ldkp, ldvp, ldo, (long long)prefix_stride, in_bf16 ? 1 : 0, out_bf16 ? 1 : 0,
                        nullptr};
    return launch_bf16<FIXED>(a, B, H, L, dh, stream);
}

int vf_attn_prefix_f32eq(const float* q, const float* k, const float* v, const float* kp, const float* vp, float* out,
                         int B, int H, int C, int N, int L, int dh, int ldq, int ldk, int ldv, int ldkp, int ldvp, int64_t prefix_stride,
                         int ldo, void* stream) {
    const prefix_args a{q, k, v, kp, vp, out, C, N, ldq, ldk, ldv, ldkp, ldvp, ldo, (long long)prefix_stride, 0, 0, nullptr};
    return launch_x6<FIXED>(a, B, H, L, dh, stream);
}

int vf_attn_prefix_var_bf16(const void* q, const void* k, const void* v, const void* kp, const void* vp, int in_bf16, void* out, int out_bf16,
                            int B, int H, int C, int N, int L, int dh, int ldq, int ldk, int ldv, int ldkp, int ldvp, int64_t prefix_stride,
                            int ldo, const int32_t* ctx_len, void* stream) {
    const prefix_args a{q, k, v, kp, vp, out, C, N, ldq, ldk, ldv, ldkp, ldvp, ldo, (long long)prefix_stride, in_bf16 ? 1 : 0, out_bf16 ? 1 : 0,
                        ctx_len};
    return launch_bf16<VAR>(a, B, H, L, dh, stream);
}

int vf_attn_prefix_var_f32eq(const float* q, const float* k, const float* v, const float* kp, const float* vp, float* out,
                             int B, int H, int C, int N, int L, int dh, int ldq, int ldk, int ldv, int ldkp, int ldvp, int64_t prefix_stride,
                             int ldo, const int32_t* ctx_len, void* stream) {
    const prefix_args a{q, k, v, kp, vp, out, C, N, ldq, ldk, ldv, ldkp, ldvp, ldo, (long long)prefix_stride, 0, 0, ctx_len};
    return launch_x6<VAR>(a, B, H, L, dh, stream);
}

int vf_attn_prefix_fork_bf16(const void* q, const void* k, const void* v, const void* kp, const void* vp, int in_bf16, void* out, int out_bf16,
                             int B, int H, int C, int N, int L, int dh, int ldq, int ldk, int ldv, int ldkp, int ldvp, int64_t prefix_stride,
                             int ldo, const int32_t* ctx_len, const void* kp2, const void* vp2, int C2, int ldkp2, int ldvp2,
                             int64_t prefix_stride2, const int32_t* split, int share, void* stream) {
    const fork_args a{{q, k, v, kp, vp, out, C, N, ldq, ldk, ldv, ldkp, ldvp, ldo, (long long)prefix_stride, in_bf16 ? 1 : 0, out_bf16 ? 1 : 0,
                       ctx_len}, kp2, vp2, C2, share, ldkp2, ldvp2, (long long)prefix_stride2, split};
    return launch_bf16<FORK>(a, B, H, L, dh, stream);
}

int vf_attn_prefix_q8_bf16(const void* q, const void* k, const void* v, const void* kq, const void* vq, const float* kscale, const float* vscale,
                           int in_bf16, void* out, int out_bf16, int B, int H, int C, int N, int L, int dh, int ldq, int ldk, int ldv,
                           int64_t q_view_stride, int64_t q_scene_stride, int64_t s_view_stride, int64_t s_scene_stride, int ldo,
                           const int32_t* ctx_len, void* stream) {
    // kp / vp of the shared checks: the packed tiles stand in (never read through them), with the tightest leading dimension
    const int ldt = H > 0 && H <= 65535 ? H * DH : 0;
    const q8_args a{{q, k, v, kq, vq, out, C, N, ldq, ldk, ldv, ldt, ldt, ldo, 0LL, in_bf16 ? 1 : 0, out_bf16 ? 1 : 0,
                     ctx_len}, (const unsigned char*)kq, (const unsigned char*)vq, kscale, vscale, (long long)q_view_stride,
                    (long long)q_scene_stride, (long long)s_view_stride, (long long)s_scene_stride};
    return launch_bf16<Q8>(a, B, H, L, dh, stream);
}

int vf_attn_prefix_fork_f32eq(const float* q, const float* k, const float* v, const float* kp, const float* vp, float* out,
                              int B, int H, int C, int N, int L, int dh, int ldq, int ldk, int ldv, int ldkp, int ldvp, int64_t prefix_stride,
                              int ldo, const int32_t* ctx_len, const float* kp2, const float* vp2, int C2, int ldkp2, int ldvp2,
                              int64_t prefix_stride2, const int32_t* split, int share, void* stream) {
    const fork_args a{{q, k, v, kp, vp, out, C, N, ldq, ldk, ldv, ldkp, ldvp, ldo, (long long)prefix_stride, 0, 0, ctx_len},
                      kp2, vp2, C2, share, ldkp2, ldvp2, (long long)prefix_stride2, split};
    return launch_x6<FORK>(a, B, H, L, dh, stream);
}

}  // extern "C"
