"""Test infrastructure of the per-kernel tests of the INFERENCE attention (tests/test_hip_infer_attention_kernels.py on the GPU,
tests/test_infer_attention_ref_host.py on the CPU): vf_attn_blockcausal_x6 (csrc/attention_x6.hip), vf_attn_blockcausal_bf16_v2's
register-staged kernel and vf_attn_blockcausal_fp8 (csrc/attention_lp.hip), vf_attn_prefix_bf16 / _f32eq and their VAR forms
(csrc/attention_prefix.hip).  vf_attn_blockcausal_f32 and the LDS-DMA kernel are the training suite's (attention_kernels_ref.py).

References.  ``attention_kernels_ref.Ref`` and ``token_mask`` give values and magnitudes; the magnitude of P is
P (1 + s_abs + sum_j P_j s_abs_j) + TINY as that module documents.  The prefix kernels take their reference as the twin-mask sequence of
C + N views with spec = C restricted to the last N views (``prefix_reference``; per-view lengths through ``mut={'vis': ...}``), and
``prefix_fp64`` is a second, independent statement written from the header text in the kernels' own layout: a separate cache addressed
by ldkp / ldvp / prefix_stride, no mask arithmetic, one softmax per (scene, view, head) over the keys the view walks.  The host test pins
the two against each other and both against oracle/migt_oracle.py.

Restatements (the roundings the sources state; rounded operands multiplied in float64, as attention_kernels_ref.fwd_bf16 does).
``fwd_x6`` is attention_kernels_ref.fwd_f32: the kernel claims fp32 equivalence and is calibrated as fp32.  ``fwd_lp`` follows
attention_lp.hip: Q, K, V rounded to bf16 UN-scaled, the score an fp32 accumulator, masked scores -1e4 / scale in units of the raw score,
m = max(raw) scale, weight p = exp2(fma(raw, c2, -m log2 e)) with c2 = scale log2 e, the normaliser summed from the UN-rounded p (the
source adds p to psum before pack8 rounds it), P = bf16(p) for the product, out = (sum P v) / l, the division last, then at most one rounding
of out to bf16.  fp8 mode: the operands clamped to +-448 and rounded to e4m3, P carried as e4m3(256 p), l multiplied by 256.

The clamp of the fp8 arm is part of the operation, not a rounding: its float64 reference is taken on the clamped operands.

Units and the fp8 floor.  unit = 2^-24 for x6 and f32eq, 2^-9 for bf16, 2^-4 for fp8 (half an ulp of e4m3's 3-bit mantissa).  TINY is
derived in attention_kernels_ref.py as (what float32 loses below its smallest normal number, 2^-126) / (its unit, 2^-24).  The same
derivation for e4m3 at the carried scale: e4m3's smallest normal number is 2^-6, its subnormals are multiples of 2^-9, so below 2^-6 the
rounding is absolute, at most half a step = 2^-10.  P is carried at 2^8: a weight below 2^-6 / 2^8 = 2^-14 is rounded with an absolute error
of at most 2^-10 / 2^8 = 2^-18, whatever its size (a weight below 2^-18 is lost whole).  In the arm's unit that is 2^-18 / 2^-4 = 2^-14
(``FLOOR8``), added to the magnitude of P for every visible key whose P is below 2^-14 (``fp8_floor``).  With it the fp8 bases of all
classes lie within one decade (0.034 'deep' .. 0.27 'large'; the host test asserts it) and the arm keeps ONE constant; the term itself
moves only the 'peaked' class, where every weight but one is under the floor (0.127 -> 0.121).

Input classes (``kind``; values are bf16-exact where the arm is bf16 or fp8): 'init' std 0.5 and 'large' std 1.0 as the training suite;
'rising' / 'falling': q and k of std 0.25 plus a shared direction u, q + 4 u and k + 8 r(j) u with r = j / T rising (resp. 1 - j / T
falling) in the key index, so that a row's running maximum moves in every 64-key tile (resp. sits in the first); 'deep': q + 6.5 u and
k - 6.5 u, every score near -42; 'peaked': q and k of std 1/16 plus 8 h_j with h_j a random sign code of unit norm per token, so that key j
leads row j by more than 20; 'largeclamp' (fp8's large case): 'large' with a few operands beyond +-448, the case on which the fp8 clamp
can be seen at all; 'wide' std 16, run at scale 2^-14 (scores as small as at scale 0.125, and -1e4 x scale = -0.6)."""
import numpy as np
import torch

import attention_kernels_ref as A
import training_kernels_ref as R
from attention_kernels_ref import DH, F32, LOG2E, U16, U32, Ref, bf, heads, rows, token_mask, view_matrix
from training_kernels_ref import F64

U8 = 2.0 ** -4
FLOOR8 = 2.0 ** -18 / U8
UNIT = {'x6': U32, 'lp': U16, 'fp8': U8, 'prefix bf16': U16, 'prefix f32eq': U32}
E4M3_MAX = 448.0
P_SCALE_FP8 = 256.0
LV = 64


def _f(x):
    return torch.tensor(float(x), dtype=F32)


# ------------------------------------------------------------------ input classes
def _noise(shape, seed, std):
    return R.normal(shape, seed, std)


def class_inputs(B, H, T, kind, seed, exact16):
    """-> q, k, v rows [B*T][H*64] float32 of class ``kind`` (bf16-exact when ``exact16``)"""
    hs = (B, H, T, DH)
    v = _noise(hs, seed + 2, 1.0)
    if kind in ('init', 'large', 'largeclamp', 'wide'):
        std = {'init': 0.5, 'wide': 16.0}.get(kind, 1.0)
        q, k = _noise(hs, seed, std), _noise(hs, seed + 1, std)
        if kind == 'largeclamp':                                                # beyond e4m3's finite range: v in three places, q in one row per head
            q, v = q.clone(), v.clone()
            for h in range(H):
                v[0, h, 3, 5], v[0, h, T // 2, 17], v[B - 1, h, T - 2, 40] = 1000.0, -640.0, 512.0
                q[0, h, T - 5, 9] = 520.0
    else:
        u = torch.full((DH,), 0.125)                                            # |u| = 1
        j = torch.arange(T, dtype=F32).reshape(1, 1, T, 1)
        if kind in ('rising', 'falling'):
            r = j / T if kind == 'rising' else 1.0 - j / T
            q = _noise(hs, seed, 0.25) + 4.0 * u
            k = _noise(hs, seed + 1, 0.25) + 8.0 * r * u
        elif kind == 'deep':
            q = _noise(hs, seed, 0.25) + 6.5 * u
            k = _noise(hs, seed + 1, 0.25) - 6.5 * u
        elif kind == 'peaked':
            code = torch.from_numpy(R.rng(seed + 3).integers(0, 2, size=hs).astype(np.float32)) * 2.0 - 1.0
            q = _noise(hs, seed, 1.0 / 16) + code
            k = _noise(hs, seed + 1, 1.0 / 16) + code
        else:
            raise ValueError(kind)
    q, k, v = (rows(x).contiguous() for x in (q, k, v))
    if exact16:
        q, k, v = (x.to(torch.bfloat16).float() for x in (q, k, v))
    return q, k, v


# ------------------------------------------------------------------ block-causal cases
# (name, B, H, T, L, spec, scale, kind).  The rate-0 rows of the training suite's F32_CASES as they are (ragged T — T = 129 is also one row
# past x6's 128-query block —, L in {0, 7, 16, 48, 96, 128, 64}, twin with 0 / interior / last / beyond views, streams on ragged and on
# 64-token views), then what the inference kernels add.
BC_CASES = [(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[8]) for c in A.F32_CASES if c[7] == 0.0] + [
    ('T100 none deep', 1, 2, 100, 0, -1, 1.0, 'deep'),                           # a zero-filled key beyond T would own every row
    ('T257 L64 causal', 1, 2, 257, 64, -1, 1.0, 'init'),                         # one row into a second 256-query workgroup of the lp kernel
    ('T320 L64 twin3 rising', 1, 2, 320, 64, 3, 1.0, 'rising'),
    ('T320 L64 twin3 falling', 1, 2, 320, 64, 3, 1.0, 'falling'),
    ('T320 L64 twin3 peaked', 1, 2, 320, 64, 3, 1.0, 'peaked'),
    ('T240 L48 causal rising', 1, 2, 240, 48, -1, 1.0, 'rising'),
    ('T240 L48 causal falling', 1, 2, 240, 48, -1, 1.0, 'falling'),
    ('T240 L48 causal peaked', 1, 2, 240, 48, -1, 1.0, 'peaked'),
    ('T144 L48 causal s2^-14', 1, 2, 144, 48, -1, 2.0 ** -14, 'wide'),           # a masked score of -1e4 x scale would weigh e^-0.6 here
]
BC_BY_NAME = {c[0]: c for c in BC_CASES}
FP8_LARGE = 'T256 L64 causal large'                                              # the fp8 arm runs this case as 'largeclamp'
# the lp kernel's four in / out dtype forms run on these; every other case runs bf16 in / fp32 out and fp32 in / bf16 out
LP_ALL_FORMS = ('T144 L48 causal s1.7', 'T256 L64 twin3', 'T256 L64 streams2x2 s1.7', 'T240 L16 streams3x5 s.125', 'T70 L7 twin8')
LP_FORMS = [(1, 0), (0, 1), (1, 1), (0, 0)]                                      # (in_bf16, out_bf16)
SPLIT_CASE = 'T144 L48 causal s1.7'                                              # operands in separate buffers with different leading dimensions


def lp_forms(name):
    return LP_FORMS if name in LP_ALL_FORMS else LP_FORMS[:2]


def bc_seed(case):
    name, B, H, T, L, spec, scale, kind = case
    return 9000 + 13 * T + 5 * H + (L + 1) * (spec + 40) + sum(map(ord, name))


def bc_inputs(case, arm):
    """-> q, k, v rows [B*T][H*64] float32; ``arm``: 'x6' (any float32), 'lp' (bf16-exact), 'fp8' (bf16-exact; its large case with
    operands beyond +-448)"""
    name, B, H, T, L, spec, scale, kind = case
    if arm == 'fp8' and name == FP8_LARGE:
        kind = 'largeclamp'
    return class_inputs(B, H, T, kind, bc_seed(case), arm != 'x6')


def clamp8(x):
    return x.clamp(-E4M3_MAX, E4M3_MAX)


def fp8_floor(q, k, v, B, H, T, L, spec, scale, vis=None):
    """the additive term of out's magnitude in the fp8 arm: sum over visible keys whose P is below 2^-14 of FLOOR8 |v| -> rows"""
    qh, kh, vh = (heads(x, B, H, T) for x in (q, k, v))
    s = float(np.float32(scale)) * (qh @ kh.transpose(-1, -2))
    vis = token_mask(T, L, spec) if vis is None else vis
    if vis is not None:
        s = s * vis.to(F64) - 1e4 * (1 - vis.to(F64))
    P = torch.softmax(s, -1)
    small = P < 2.0 ** -14
    if vis is not None:
        small &= vis
    return rows((small.to(F64) * FLOOR8) @ vh.abs())


def bc_reference(case, arm, mut=None, inputs=None):
    """-> (Ref, (out value, out magnitude)) of a block-causal case for ``arm``"""
    name, B, H, T, L, spec, scale, kind = case
    q, k, v = bc_inputs(case, arm) if inputs is None else inputs
    if arm == 'fp8':
        q, k, v = clamp8(q), clamp8(k), clamp8(v)
    ref = Ref(q, k, v, None, B, H, T, L, spec, scale, mut=mut)
    val, mag = ref.out
    if arm == 'fp8':
        mag = mag + fp8_floor(q, k, v, B, H, T, L, spec, scale, vis=(mut or {}).get('vis'))
    return ref, (val, mag)


# ------------------------------------------------------------------ restatements
def fwd_x6(q, k, v, B, H, T, L, spec, scale):
    return A.fwd_f32(q, k, v, B, H, T, L, spec, scale)[0]


def e4m3(x, saturating_cast=False):
    """round to OCP e4m3 as v_cvt_pk_fp8_f32 does, back in float64: the instruction does not saturate (attention_lp.hip: pack8), a finite
    value beyond the format's range becomes NaN"""
    x32 = x.to(F32)
    y = x32.to(torch.float8_e4m3fn).to(F64)
    return torch.where(x32.abs() > 464.0, torch.full_like(y, float('nan')), y)    # 464 = the midpoint above 448 rounds up out of the format


def _lp_core(qh, kh, vh, vis, scale, fp8, out_bf16):
    """one (batch of) head(s): qh [.., Tq, 64] already rounded (float64), kh / vh [.., Tk, 64], vis bool [Tq][Tk] or None"""
    sc = _f(scale)
    s = (qh @ kh.transpose(-1, -2)).to(F32)                                     # fp32 accumulator of exact products
    if vis is not None:
        s = torch.where(vis, s, _f(-1e4) / sc)
    m = s.max(-1, keepdim=True).values * sc
    c2, mc = sc * _f(LOG2E), m * _f(LOG2E)
    p = torch.exp2((s.to(F64) * c2.to(F64) - mc.to(F64)).to(F32))               # one fma, one exp2
    l = p.to(F64).sum(-1, keepdim=True).to(F32)                                 # psum takes p before its rounding
    if fp8:
        pk, l = e4m3(p * _f(P_SCALE_FP8)), l * _f(P_SCALE_FP8)
    else:
        pk = bf(p)
    o = (pk @ vh).to(F32) / l
    return bf(o) if out_bf16 else o.to(F64)


def fwd_lp(q, k, v, B, H, T, L, spec, scale, out_bf16=False, fp8=False, clamp=True, vis=None):
    """attention_lp.hip (module docstring) -> out rows, float64 of the float32 / bf16 values.  ``clamp`` False: the fp8 mutant."""
    rnd = (lambda x: e4m3(clamp8(x) if clamp else x)) if fp8 else bf
    qh, kh, vh = (rnd(heads(x, B, H, T, F32)) for x in (q, k, v))
    vis = token_mask(T, L, spec) if vis is None else vis
    return rows(_lp_core(qh, kh, vh, vis, scale, fp8, out_bf16))


# ------------------------------------------------------------------ prefix cases
# (name, B, C, N, kind, layout, lens): H = 2, L = 64.  N around the group sizes (4 views per workgroup in the bf16 arm, 2 in f32eq): full
# groups, partial last groups, single views.  layout 'fused': the cache is the K and V thirds of the context's [B*C*L][3d + pad] c_attn
# buffer; 'kv': kp and vp in separate buffers with ldkp != ldvp != ldq; 'stride': fused with prefix_stride beyond one scene's extent.
# lens: per-view context lengths [B][N] (VAR entries; cache rows at or beyond a view's length are NaN on the GPU) or None (fixed C).
PREFIX_CASES = [
    ('B1 C1 N1', 1, 1, 1, 'init', 'fused', None),
    ('B2 C1 N5', 2, 1, 5, 'init', 'kv', None),
    ('B2 C2 N3', 2, 2, 3, 'init', 'fused', None),
    ('B2 C2 N3 rising', 2, 2, 3, 'rising', 'fused', None),
    ('B2 C2 N3 peaked', 2, 2, 3, 'peaked', 'fused', None),
    ('B1 C3 N4', 1, 3, 4, 'init', 'stride', None),
    ('B1 C3 N4 deep', 1, 3, 4, 'deep', 'fused', None),
    ('B2 C5 N2', 2, 5, 2, 'init', 'fused', None),
    ('B1 C19 N2', 1, 19, 2, 'init', 'fused', None),                              # the largest: (C + N) x 64 = 1344 tokens
    # VAR.  bf16: a workgroup holds views {1, 4} / {0, 0} resp. {3, 0, 2, 1}; f32eq: {1, 4} / {0, 0} resp. {3, 0} / {2, 1}
    ('B2 C5 N2 var', 2, 5, 2, 'init', 'fused', ((1, 4), (0, 0))),
    ('B1 C3 N4 var', 1, 3, 4, 'init', 'kv', ((3, 0, 2, 1),)),
]
PREFIX_BY_NAME = {c[0]: c for c in PREFIX_CASES}
PREFIX_H = 2


def prefix_inputs(case, exact16):
    """one sequence of C + N views per scene in class ``kind``, split as the renderer holds it -> dict q, k, v rows [B*N*L][d] and
    kp, vp [B][C*L][d] float32"""
    name, B, C, N, kind, layout, lens = case
    H, T, d = PREFIX_H, (C + N) * LV, PREFIX_H * DH
    q, k, v = class_inputs(B, H, T, kind, 11000 + 17 * C + 3 * N + B + sum(map(ord, name)), exact16)
    q, k, v = (x.reshape(B, T, d) for x in (q, k, v))
    own = slice(C * LV, T)
    return dict(q=q[:, own].reshape(B * N * LV, d).contiguous(), k=k[:, own].reshape(B * N * LV, d).contiguous(),
                v=v[:, own].reshape(B * N * LV, d).contiguous(), kp=k[:, :C * LV].contiguous(), vp=v[:, :C * LV].contiguous())


def prefix_sequence(x, B, C, N):
    """the concatenated sequences of the twin-mask pass -> q, k, v rows [B*(C+N)*L][d] (the prefix's queries are zeros: their rows are
    not compared)"""
    d = x['q'].shape[1]
    T = (C + N) * LV

    def cat(pre, own):
        return torch.cat([pre, own.reshape(B, N * LV, d)], 1).reshape(B * T, d)
    return cat(torch.zeros_like(x['kp']), x['q']), cat(x['kp'], x['k']), cat(x['vp'], x['v'])


def prefix_vis(C, N, lens_b):
    """token mask [T][T] of one scene's concatenated sequence: query view C + n sees prefix views < lens_b[n] and itself"""
    nv = C + N
    vm = view_matrix(nv, C).clone()
    for n in range(N):
        vm[C + n, :C] = torch.arange(C) < int(lens_b[n])
    return token_mask(nv * LV, LV, C, views=vm)


def prefix_reference(case, exact16, lens='case', inputs=None):
    """(value, magnitude) rows [B*N*L][d]: attention_kernels_ref.Ref on the twin-mask sequence, the last N views"""
    name, B, C, N, kind, layout, lens0 = case
    lens = lens0 if isinstance(lens, str) else lens
    x = prefix_inputs(case, exact16) if inputs is None else inputs
    H, T, d = PREFIX_H, (C + N) * LV, PREFIX_H * DH
    qs, ks, vs = prefix_sequence(x, B, C, N)
    vals, mags = [], []
    for b in range(B):                                                          # (lengths differ per scene: one Ref per scene)
        sl = slice(b * T, (b + 1) * T)
        mut = None if lens is None else {'vis': prefix_vis(C, N, lens[b])}
        val, mag = Ref(qs[sl], ks[sl], vs[sl], None, 1, H, T, LV, C, 1.0, mut=mut).out
        vals.append(val[C * LV:])
        mags.append(mag[C * LV:])
    return torch.cat(vals), torch.cat(mags)


def prefix_fp64(q, k, v, kp, vp, B, H, C, N, ldkp, ldvp, prefix_stride, lens=None):
    """the header's statement in the kernels' layout: q / k / v rows [B*N*L][>= H*64]; kp / vp FLAT buffers, key row r of scene b and head h
    at element b prefix_stride + r ld + 64 h.  View (b, n) attends to the first len(b, n) L rows of its scene's cache and to the L keys of
    its own view, nothing else; un-scaled scores, softmax, times v -> out rows [B*N*L][H*64] float64"""
    out = torch.zeros((B * N * LV, H * DH), dtype=F64)
    for b in range(B):
        for n in range(N):
            c = C if lens is None else min(max(int(lens[b][n]), 0), C)
            r0 = (b * N + n) * LV
            for h in range(H):
                col = slice(h * DH, (h + 1) * DH)
                keys, vals = [], []
                for r in range(c * LV):
                    ko, vo = b * prefix_stride + r * ldkp + h * DH, b * prefix_stride + r * ldvp + h * DH
                    keys.append(kp[ko:ko + DH])
                    vals.append(vp[vo:vo + DH])
                K = torch.stack(keys + list(k[r0:r0 + LV, col])).to(F64)
                V = torch.stack(vals + list(v[r0:r0 + LV, col])).to(F64)
                w = q[r0:r0 + LV, col].to(F64) @ K.T
                w = torch.exp(w - w.max(-1, keepdim=True).values)
                out[r0:r0 + LV, col] = (w / w.sum(-1, keepdim=True)) @ V
    return out


def prefix_restate(arm, x, B, C, N, lens=None, out_bf16=False):
    """the prefix kernels' arithmetic per (scene, view): arm 'prefix bf16' = attention_lp.hip's with scale 1 over the keys the view walks,
    'prefix f32eq' = float32 softmax attention (calibrated as fp32, as x6) -> out rows"""
    H, d = PREFIX_H, PREFIX_H * DH
    out = torch.zeros((B * N * LV, d), dtype=F64)
    for b in range(B):
        for n in range(N):
            c = C if lens is None else int(lens[b][n])
            r0 = (b * N + n) * LV
            sl = slice(r0, r0 + LV)
            kk = torch.cat([x['kp'][b, :c * LV], x['k'][sl]])
            vv = torch.cat([x['vp'][b, :c * LV], x['v'][sl]])
            Tk = kk.shape[0]
            qh = x['q'][sl].reshape(LV, H, DH).permute(1, 0, 2)
            kh, vh = kk.reshape(Tk, H, DH).permute(1, 0, 2), vv.reshape(Tk, H, DH).permute(1, 0, 2)
            if arm == 'prefix bf16':
                o = _lp_core(bf(qh), bf(kh), bf(vh), None, 1.0, False, out_bf16)
            else:
                s = qh.to(F32) @ kh.to(F32).transpose(-1, -2)
                m = s.max(-1, keepdim=True).values
                p = torch.exp2((s - m) * _f(LOG2E))
                o = ((p @ vh.to(F32)) / p.sum(-1, keepdim=True)).to(F64)
            out[sl] = o.permute(1, 0, 2).reshape(LV, d)
    return out


# ------------------------------------------------------------------ mutants that are not a mask
def out_rescale_skipped(q, k, v, B, H, T, L, spec, scale):
    """float64 out of a kernel that never rescales its accumulator: tile t's products enter with exp(s - m_t), m_t the running maximum
    after tile t, while the normaliser is the correct one (taken at the final maximum)"""
    qh, kh, vh = (heads(x, B, H, T) for x in (q, k, v))
    s = float(np.float32(scale)) * (qh @ kh.transpose(-1, -2))
    vis = token_mask(T, L, spec)
    if vis is not None:
        s = s * vis.to(F64) - 1e4 * (1 - vis.to(F64))
    m_fin = s.max(-1, keepdim=True).values
    l = torch.exp(s - m_fin).sum(-1, keepdim=True)
    acc = torch.zeros_like(qh)
    m_run = torch.full_like(m_fin, float('-inf'))
    for t0 in range(0, T, 64):
        st = s[..., t0:t0 + 64]
        m_run = torch.maximum(m_run, st.max(-1, keepdim=True).values)
        acc = acc + torch.exp(st - m_run) @ vh[..., t0:t0 + 64, :]
    return rows(acc / l)


def tile_maxima(q, k, B, H, T, L, spec, scale):
    """per row, the maximum visible score of each 64-key tile (-inf where the tile holds no visible key) -> [B][H][T][ntiles] float64"""
    qh, kh = heads(q, B, H, T), heads(k, B, H, T)
    s = float(np.float32(scale)) * (qh @ kh.transpose(-1, -2))
    vis = token_mask(T, L, spec)
    if vis is not None:
        s = torch.where(vis, s, torch.full_like(s, float('-inf')))
    nt = (T + 63) // 64
    s = torch.nn.functional.pad(s, (0, nt * 64 - T), value=float('-inf'))
    return s.reshape(B, H, T, nt, 64).max(-1).values
