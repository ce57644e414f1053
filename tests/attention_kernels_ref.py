"""Test infrastructure of the per-kernel tests of the training attention (tests/test_hip_attention_kernels.py on the GPU,
tests/test_attention_kernels_ref_host.py on the CPU): the six entry points vf_attn_blockcausal_lse_f32 / vf_attn_bwd_prep_f32 /
vf_attn_bwd_f32 and vf_attn_blockcausal_bf16_lse / vf_attn_bwd_prep_bf16 / vf_attn_bwd_bf16.

References.  float64, written from the definition in include/vf_hip.h in the kernels' own layout (rows [B*T][ld], head h at column h*64):
score s = scale q.k, masked entries take -1e4 exactly as ``w*m - 1e4*(1-m)``, visibility = vf_attn_visible restated (``visible`` scalar,
``view_matrix`` vectorised), L = 0 = no mask; lse = log sum_k exp(s) before dropout, P = exp(s - lse), out = sum_k keep c P v with
c = 1/(1-rate) (the float32 value the kernels use), D = rowsum(dO O), dP = keep c (dO.v), dS = P (dP - D) scale, dq = dS k, dk = dS^T q,
dv = (keep c P)^T dO: sums written out, autograd only pins them (host test).  The dropout mask restates viewformer_amd/_hash.py
(``attn_group``, ``dropout_keep``) with drop_plane0 added to the plane.

Magnitudes.  Every reference returns ``(value, magnitude)``, the magnitude being the same expression with every summand replaced by its
absolute value, with one addition that the plain rule misses.  Every term of a softmax is positive, so the plain rule gives P itself; but
exp carries the ABSOLUTE error of its argument into P as a relative error.  The argument s - lse is a 64-term sum whose rounding (float32:
of the products; bf16 arm: of q' = bf16(q scale log2 e), 2^-9 per element) is bounded by unit x s_abs, s_abs = scale |q|.|k|, and lse
inherits the P-weighted mean of the same.  So the magnitude of P is
    P (1 + s_abs + sum_j P_j s_abs_j)         (+ 2^-126 / 2^-24 where P is below float32's smallest normal number)
and out, dq, dk, dv use it wherever their expression holds P.  lse itself: its stated roundings are the score's (sum_j P_j s_abs_j, in the
arm's unit) and those of a float32 sum, its logarithm and the float32 it is stored as, which cost 2^-24 (|lse| + 1) in BOTH arms (the 1: the
relative error of the summed exponentials is an absolute error of their logarithm).  In the arm's unit that is
    sum_j P_j s_abs_j + (|lse| + 1) 2^-24 / unit
i.e. |lse| + 1 + sum_j P_j s_abs_j for the f32 kernels, and the score term almost alone for the bf16 forward: judged against |lse| + 1 in
units of 2^-9 its lse would be allowed 140 times its own rounding error at scale 0.125.  With these terms the calibration bases of the
bf16 arm (out, lse, dq, dk, dv) stay within one decade between the smallest scores of the list (scale 0.125: s_abs ~ 1) and the
large-score case (s_abs ~ 40) — the host test prints them per case and asserts the decade; under the plain rule the bases of out run from
1.0 to 22.  The unit is 2^-24 for the f32 kernels and 2^-9 for the bf16 kernels (``ratio``).

Restatements.  ``*_f32``: the kernel's formula on CPU float32 ops (exp2((s - lse) log2 e) as written).  ``*_bf16``: the roundings the
sources state — q' = bf16(q scale log2 e) in the forward and the dQ kernel, the un-folded fp32 score times scale log2 e in the dK / dV
kernel, P and dS rounded to bf16 before their products, dropout on the rounded P, out rounded once, D from bf16 out / dout in fp32,
gradients fp32 or rounded once — with the products of rounded operands in float64: they measure what the stated roundings cost, not the
MFMA's summation order.  The GPU test's constants are 4 x the worst restatement error, rounded up to a power of two."""
import numpy as np
import torch

import training_kernels_ref as R
from training_kernels_ref import F64, t64

U32, U16 = 2.0 ** -24, 2.0 ** -9
LOG2E = np.float32(1.4426950408889634)
LN2 = np.float32(0.69314718055994531)
TINY = 2.0 ** -126 / 2.0 ** -24
DH = 64
SEED, SITE = 20231, 16                                                          # dropout (seed, site) of every case that drops


def ratio(got, want, mag, unit):
    """R.worst_ratio in units of ``unit`` x magnitude"""
    return R.worst_ratio(got, want, mag) * (U32 / unit)


def rejects(got, want, mag, c, unit):
    return not ratio(got, want, mag, unit) <= c


# ------------------------------------------------------------------ visibility
def visible(qv, kv, spec):
    """vf_attn_visible (csrc/vf_common.h): plain (-1) / twin (Vc = spec >= 0) / streams (Sv = -spec >= 2)"""
    if spec <= -2:
        Sv = -spec
        qs, qi, ks, ki = qv // Sv, qv % Sv, kv // Sv, kv % Sv
        return (ks == 0 and ki <= qi) if qs == 0 else ((ks == 0 and ki < qi) or kv == qv)
    Vc = spec if spec >= 0 else 0x3fffffff
    return kv == qv or min(kv, Vc) < min(qv, Vc)


def view_matrix(nviews, spec, device=None):
    """bool [query view][key view]"""
    qv = torch.arange(nviews, device=device)[:, None]
    kv = torch.arange(nviews, device=device)[None, :]
    if spec <= -2:
        Sv = -spec
        qs, qi, ks, ki = qv // Sv, qv % Sv, kv // Sv, kv % Sv
        return torch.where(qs == 0, (ks == 0) & (ki <= qi), ((ks == 0) & (ki < qi)) | (kv == qv))
    Vc = spec if spec >= 0 else 0x3fffffff
    return (kv == qv) | (kv.clamp(max=Vc) < qv.clamp(max=Vc))


def token_mask(T, L, spec, device=None, views=None):
    """bool [T][T] over tokens (view = token // L), None when L = 0; ``views``: a view matrix to use instead of the spec's"""
    if L == 0:
        return None
    nv = (T + L - 1) // L
    vm = view_matrix(nv, spec, device) if views is None else views.to(device)
    tv = torch.arange(T, device=device) // L
    return vm[tv][:, tv]


# ------------------------------------------------------------------ dropout
def drop_c(rate):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))


def attn_groups(plane, T, stride=None):
    """(group, position) of attention weight (plane, q, k) for all q, k of a T-token sequence, written out from the definition in
    viewformer_amd/_hash.py: group = plane << 32 | (q ceil(T/4) + (k >> 2)), position = k & 3.  ``stride`` replaces ceil(T/4) (mutants)"""
    q = np.arange(T, dtype=np.uint64)[:, None]
    k = np.arange(T, dtype=np.uint64)[None, :]
    stride = np.uint64((T + 3) // 4 if stride is None else stride)
    g = (np.uint64(plane) << np.uint64(32)) | (q * stride + (k >> np.uint64(2)))
    return g, np.broadcast_to(k & np.uint64(3), g.shape)


def keep_mask(B, H, T, rate, seed=SEED, site=SITE, plane0=0, stride=None):
    """float64 {0, 1} [B][H][T][T]: element (b, h, q, k) is kept iff dropout_keep(word of its group in plane plane0 + b H + h, k & 3) with
    the hashed words of viewformer_amd/_hash.py; None when rate = 0"""
    if not rate:
        return None
    from viewformer_amd import _hash as hh
    rate = float(np.float32(rate))                                              # the float the entry point receives
    planes = [hh.dropout_keep(seed, site, *attn_groups(plane0 + p, T, stride), rate) for p in range(B * H)]
    return torch.from_numpy(np.stack(planes).reshape(B, H, T, T).astype(np.float64))


# ------------------------------------------------------------------ layout
def heads(x, B, H, T, dtype=F64):
    """rows [B*T][>= H*64] -> [B][H][T][64]"""
    x = x if torch.is_tensor(x) else torch.as_tensor(x)
    return x[:, :H * DH].to(dtype).reshape(B, T, H, DH).permute(0, 2, 1, 3)


def rows(x):
    """[B][H][T][64] -> rows [B*T][H*64]"""
    B, H, T, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * DH)


# ------------------------------------------------------------------ float64 references
class Ref:
    """the references of one case, computed once: ``lse``, ``out``, ``D``, ``dq``, ``dk``, ``dv`` are (value, magnitude) pairs in the
    kernels' layouts ([B][H][T] for lse and D, rows [B*T][H*64] otherwise).  ``mut`` (mutants of the host test): 'vis' a token mask to use,
    'no_scale_score' / 'no_scale_dq' / 'no_scale_dk', 'no_D_rows' (r0, r1): the D term dropped for those queries, 'dv_no_c',
    'lse_after_dropout', 'plain_magnitude' (the magnitude of P without its score term).  ``unit``: the unit the comparison will use (2^-24 or
    2^-9): only the magnitude of lse depends on it."""

    def __init__(self, q, k, v, dout, B, H, T, L, spec, scale, keep=None, c=1.0, mut=None, device=None, unit=U32):
        mut = mut or {}
        dev = device
        qh, kh, vh = (heads(torch.as_tensor(x).to(dev), B, H, T) for x in (q, k, v))
        sc = float(np.float32(scale))
        s = (1.0 if 'no_scale_score' in mut else sc) * (qh @ kh.transpose(-1, -2))
        sa = sc * (qh.abs() @ kh.abs().transpose(-1, -2))
        vis = mut['vis'].to(dev) if 'vis' in mut else token_mask(T, L, spec, dev)
        if vis is not None:
            m = vis.to(F64)
            s = s * m - 1e4 * (1 - m)
            sa = sa * m
        self.row_max = s.max(-1).values
        lse = torch.logsumexp(s, -1)
        P = torch.exp(s - lse[..., None])
        del s
        e = (P * sa).sum(-1)
        Pm = P * (1.0 + sa + e[..., None]) if 'plain_magnitude' not in mut else P.clone()
        del sa
        small = P < 2.0 ** -126
        if vis is not None:
            small &= vis
        Pm += small.to(F64) * TINY
        kc = None if keep is None else keep.to(dev) * c
        # lse: the score term e in the arm's unit; |lse| + 1 (the float32 sum, its logarithm, the stored float32) always costs 2^-24
        lse_mag = e + (lse.abs() + 1.0) * (U32 / unit)
        if 'lse_after_dropout' in mut and kc is not None:
            self.lse = (torch.log((kc * P).sum(-1)) + lse, lse_mag)
        else:
            self.lse = (lse, lse_mag)
        Pd = P if kc is None else kc * P
        Pdm = Pm if kc is None else kc * Pm
        O = Pd @ vh
        self.out = (rows(O), rows(Pdm @ vh.abs()))
        if dout is None:
            return
        doh = heads(torch.as_tensor(dout).to(dev), B, H, T)
        D = (doh * O).sum(-1)
        self.D = (D, (doh.abs() * O.abs()).sum(-1))
        Da = (doh.abs() * (Pd @ vh.abs())).sum(-1)
        dP = doh @ vh.transpose(-1, -2)
        dPa = doh.abs() @ vh.abs().transpose(-1, -2)
        if kc is not None:
            dP, dPa = kc * dP, kc * dPa
        Dd = D.clone()
        if 'no_D_rows' in mut:
            Dd[..., mut['no_D_rows'][0]:mut['no_D_rows'][1]] = 0.0
        dS1 = P * (dP - Dd[..., None])                                          # dS / scale
        dSm = Pm * (dPa + Da[..., None]) * sc
        del dP, dPa
        self.dq = (rows(((1.0 if 'no_scale_dq' in mut else sc) * dS1) @ kh), rows(dSm @ kh.abs()))
        self.dk = (rows(((1.0 if 'no_scale_dk' in mut else sc) * dS1).transpose(-1, -2) @ qh), rows(dSm.transpose(-1, -2) @ qh.abs()))
        del dS1, dSm
        Pv = P if ('dv_no_c' in mut or kc is None) else Pd
        if 'dv_no_c' in mut and keep is not None:
            Pv = keep.to(dev) * P
        self.dv = (rows(Pv.transpose(-1, -2) @ doh), rows(Pdm.transpose(-1, -2) @ doh.abs()))


def rowsum_D(dout, out, B, H, T):
    """D = rowsum(dO O) of the ``out`` it is given -> ([B][H][T], magnitude)"""
    a, o = heads(dout, B, H, T), heads(out, B, H, T)
    return (a * o).sum(-1), (a.abs() * o.abs()).sum(-1)


# ------------------------------------------------------------------ restatements of the kernels' formulas
F32 = torch.float32


def _f(x):
    return torch.tensor(float(x), dtype=F32)


def _vis_f(T, L, spec):
    return token_mask(T, L, spec)


def fwd_f32(q, k, v, B, H, T, L, spec, scale, keep=None, c=1.0):
    """attention_f32.hip: s = (q.k) scale, masked -1e4, p = exp2((s - m) log2 e), the normaliser over the undropped weights,
    out = (sum keep c p v) / l, lse = m + log l -> (out rows, lse [B][H][T])"""
    qh, kh, vh = (heads(x, B, H, T, F32) for x in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * _f(scale)
    vis = _vis_f(T, L, spec)
    if vis is not None:
        s = torch.where(vis, s, _f(-1e4))
    m = s.max(-1, keepdim=True).values
    p = torch.exp2((s - m) * _f(LOG2E))
    l = p.sum(-1, keepdim=True)
    pd = p if keep is None else torch.where(keep > 0, p * _f(c), _f(0.0))
    return rows((pd @ vh) / l), (m + torch.log(l)).squeeze(-1)


def prep_f32(dout, out, B, H, T):
    return (heads(dout, B, H, T, F32) * heads(out, B, H, T, F32)).sum(-1)


def bwd_f32(q, k, v, dout, lse, D, B, H, T, L, spec, scale, keep=None, c=1.0):
    """attention_bwd_f32.hip: p = exp2((s - lse) log2 e), dS = p (keep c dP - D) scale -> (dq, dk, dv) rows"""
    qh, kh, vh, doh = (heads(x, B, H, T, F32) for x in (q, k, v, dout))
    s = (qh @ kh.transpose(-1, -2)) * _f(scale)
    vis = _vis_f(T, L, spec)
    if vis is not None:
        s = torch.where(vis, s, _f(-1e4))
    p = torch.exp2((s - lse.to(F32)[..., None]) * _f(LOG2E))
    dp = doh @ vh.transpose(-1, -2)
    pd = p
    if keep is not None:
        dp = torch.where(keep > 0, dp * _f(c), _f(0.0))
        pd = torch.where(keep > 0, p * _f(c), _f(0.0))
    ds = p * (dp - D.to(F32)[..., None]) * _f(scale)
    return rows(ds @ kh), rows(ds.transpose(-1, -2) @ qh), rows(pd.transpose(-1, -2) @ doh)


def bf(x):
    """round to bf16 (through float32, as the kernels hold the value), back in float64"""
    return x.to(F32).to(torch.bfloat16).to(F64)


def _folded_q(qh32, scale):
    return bf(qh32 * (_f(scale) * _f(LOG2E)))                                  # q' = bf16(q * (scale * log2 e)), the product in fp32


def fwd_bf16(q, k, v, B, H, T, spec, scale, keep=None, c=1.0, unrounded_q=False):
    """attention_dma.hip with lse: S2 = k.q' in log2 units (fp32 accumulator), invisible tiles skipped, p = exp2(S2 - m), normaliser
    over the unrounded undropped p, pk = bf16(keep ? p : 0), out = bf16((sum pk v) (c / l)), lse = m ln 2 + log l.
    -> (out rows as float64 of bf16 values, lse [B][H][T] float32).  ``unrounded_q`` (mutant): P from q scale log2 e without its
    rounding."""
    qh, kh, vh = heads(q, B, H, T, F32), heads(k, B, H, T), heads(v, B, H, T)
    q1 = (qh * (_f(scale) * _f(LOG2E))).to(F64) if unrounded_q else _folded_q(qh, scale)
    s2 = (q1 @ kh.transpose(-1, -2)).to(F32)
    vis = token_mask(T, DH, spec)
    s2 = torch.where(vis, s2, _f(float('-inf')))
    m = s2.max(-1, keepdim=True).values
    p = torch.exp2(s2 - m)
    l = p.to(F64).sum(-1, keepdim=True).to(F32)
    pk = bf(p if keep is None else torch.where(keep > 0, p, _f(0.0)))
    o = (pk @ vh).to(F32) * (_f(c) / l)
    return rows(bf(o)), (m * _f(LN2) + torch.log(l)).squeeze(-1)


def prep_bf16(dout, out, B, H, T):
    return (heads(dout, B, H, T) * heads(out, B, H, T)).sum(-1).to(F32)


def bwd_bf16(q, k, v, dout, lse, D, B, H, T, spec, scale, keep=None, c=1.0, out_bf16=False):
    """attention_train_bf16.hip.  dQ kernel: S2 = k.q' + (log2 scale - lse log2 e), ps = exp2(S2) = scale P, x = dP - D (dropout:
    keep ? c dP - D : -D), dS = bf16(ps x), dq = dS.k.  dK / dV kernel: p = exp2(fma(q.k, scale log2 e, -lse log2 e)) from the UN-folded
    q, P = bf16(keep ? p : 0), dS = bf16(p (dP - D) scale) (dropout: fma(keep p, dP c scale, -(p (D scale)))), dv = (P^T.dO) c,
    dk = dS^T.q.  -> (dq, dk, dv) rows, float32 values (bf16 values when ``out_bf16``)"""
    qh32 = heads(q, B, H, T, F32)
    qh, kh, vh, doh = (heads(x, B, H, T) for x in (q, k, v, dout))
    lse32, D32 = lse.to(F32)[..., None], D.to(F32)[..., None]
    vis = token_mask(T, DH, spec)
    dp = (doh @ vh.transpose(-1, -2)).to(F32)
    sc, cf = _f(scale), _f(c)
    # dQ
    cs = torch.log2(sc) - lse32 * _f(LOG2E)
    st = ((_folded_q(qh32, scale) @ kh.transpose(-1, -2)) + cs.to(F64)).to(F32)
    ps = torch.where(vis, torch.exp2(st), _f(0.0))
    if keep is None:
        x = (dp.to(F64) - D32.to(F64)).to(F32)
    else:
        x = torch.where(keep > 0, (dp.to(F64) - (D32 / cf).to(F64)).to(F32) * cf, -D32.expand_as(dp))
    dq = bf(ps * x) @ kh
    # dK, dV
    s = (qh @ kh.transpose(-1, -2)).to(F32)
    p = torch.where(vis, torch.exp2(s * (sc * _f(LOG2E)) - lse32 * _f(LOG2E)), _f(0.0))
    if keep is None:
        pf, sf = bf(p), bf(p * (dp - D32) * sc)
        dv = (pf.transpose(-1, -2) @ doh).to(F32)
    else:
        pk = torch.where(keep > 0, p, _f(0.0))
        pf, sf = bf(pk), bf(pk * (dp * (cf * sc)) - p * (D32 * sc))
        dv = (pf.transpose(-1, -2) @ doh).to(F32) * cf
    dk = sf.transpose(-1, -2) @ qh
    res = tuple(rows(g.to(F32)) for g in (dq, dk, dv))
    return tuple(bf(g) for g in res) if out_bf16 else res


# ------------------------------------------------------------------ cases and inputs (shared by the CPU calibration and the GPU test)
# (name, B, H, T, L, spec, scale, rate, kind): kind 'init' = q, k of standard deviation 0.5 (scores of a few units), 'large' = 1.0 (|s| to ~40,
# as tests/test_train.py::test_bf16_flash_attention_backward_at_trained_scale_scores generates them)
F32_CASES = [
    ('T70 none s1.7', 2, 2, 70, 0, -1, 1.7, 0.0, 'init'),                        # partial wave, partial tile, T % 4 != 0
    ('T70 none drop', 2, 2, 70, 0, -1, 1.0, 0.2, 'init'),                        # ... with dropout: group stride ceil(T/4)
    ('T129 none s.125', 1, 2, 129, 0, -1, 0.125, 0.0, 'init'),                   # one row past the 128-row owner block
    ('T70 L7 twin8', 2, 2, 70, 7, 8, 1.0, 0.0, 'init'),                          # small ragged views
    ('T144 L48 causal s1.7', 2, 2, 144, 48, -1, 1.7, 0.0, 'init'),               # L does not divide 64
    ('T240 L16 streams3x5 s.125', 1, 2, 240, 16, -5, 0.125, 0.0, 'init'),        # streams on ragged views
    ('T288 L96 causal', 1, 2, 288, 96, -1, 1.0, 0.0, 'init'),                    # L > 64, L % 64 != 0: per-element path
    ('T384 L128 causal s1.7', 1, 2, 384, 128, -1, 1.7, 0.0, 'init'),             # a view wider than a tile on the uniform path
    ('T64 L64 causal s.125', 2, 2, 64, 64, -1, 0.125, 0.0, 'init'),              # one view
    ('T256 L64 twin0', 2, 2, 256, 64, 0, 1.0, 0.0, 'init'),                      # every view sees only itself
    ('T256 L64 twin2 drop', 2, 2, 256, 64, 2, 1.0, 0.2, 'init'),
    ('T256 L64 twin3', 2, 2, 256, 64, 3, 1.0, 0.0, 'init'),                      # Vc = nviews - 1
    ('T256 L64 twin4', 2, 2, 256, 64, 4, 1.0, 0.0, 'init'),                      # Vc >= nviews: plain block-causal, bit for bit
    ('T576 L64 streams3x3 drop', 2, 2, 576, 64, -3, 1.0, 0.2, 'init'),           # the trainer's mask
    ('T256 L64 streams2x2 s1.7', 2, 2, 256, 64, -2, 1.7, 0.0, 'init'),
    ('T640 L64 streams5x2 s.125', 1, 2, 640, 64, -2, 0.125, 0.0, 'init'),
    ('T256 L64 causal large', 2, 2, 256, 64, -1, 1.0, 0.0, 'large'),             # scores spread to |s| ~ 40
]
BF16_CASES = [
    ('1 view causal', 2, 2, 64, 64, -1, 1.0, 0.0, 'init'),
    ('2 views causal s.125', 2, 2, 128, 64, -1, 0.125, 0.0, 'init'),
    ('3 views causal s1.7', 2, 2, 192, 64, -1, 1.7, 0.0, 'init'),                # the second view of the last owner block does not exist
    ('5 views twin0', 2, 2, 320, 64, 0, 1.0, 0.0, 'init'),
    ('5 views twin3 s1.7', 2, 2, 320, 64, 3, 1.7, 0.0, 'init'),
    ('5 views twin4', 2, 2, 320, 64, 4, 1.0, 0.0, 'init'),
    ('5 views twin9', 2, 2, 320, 64, 9, 1.0, 0.0, 'init'),                       # must equal spec -1
    ('9 views streams3x3 drop', 2, 2, 576, 64, -3, 1.0, 0.2, 'init'),
    ('4 views streams2x2 s.125', 2, 2, 256, 64, -2, 0.125, 0.0, 'init'),
    ('4 views causal large', 2, 2, 256, 64, -1, 1.0, 0.0, 'large'),
    ('64 views causal', 1, 1, 4096, 64, -1, 1.0, 0.0, 'init'),                   # the limit: hi >= 64 and 1ull << 63 of the closed-form masks
    ('64 views twin62', 1, 1, 4096, 64, 62, 1.0, 0.0, 'init'),
    ('64 views streams4x16', 1, 1, 4096, 64, -16, 1.0, 0.0, 'init'),
    ('64 views streams2x32', 1, 1, 4096, 64, -32, 1.0, 0.0, 'init'),
]
F32_BY_NAME = {c[0]: c for c in F32_CASES}
BF16_BY_NAME = {c[0]: c for c in BF16_CASES}
BIG_T = 4096                                                                     # cases of this T take their reference on the device


def inputs(case, bf16):
    """-> q, k, v, dout [B*T][H*64] float32 (bf16-exact values when ``bf16``)"""
    name, B, H, T, L, spec, scale, rate, kind = case
    seed = 7000 + 13 * T + 5 * H + (L + 1) * (spec + 40) + (1 if bf16 else 0) + sum(map(ord, name))
    std = 1.0 if kind == 'large' else 0.5
    q, k = R.normal((B * T, H * DH), seed, std), R.normal((B * T, H * DH), seed + 1, std)
    v, dout = R.normal((B * T, H * DH), seed + 2), R.normal((B * T, H * DH), seed + 3)
    if bf16:
        q, k, v, dout = (x.to(torch.bfloat16).float() for x in (q, k, v, dout))
    return q, k, v, dout


def case_keep(case, plane0=0):
    """-> (keep [B][H][T][T] or None, c)"""
    name, B, H, T, L, spec, scale, rate, kind = case
    return keep_mask(B, H, T, rate, plane0=plane0), (drop_c(rate) if rate else 1.0)


def reference(case, bf16, device=None, mut=None, keep='case'):
    q, k, v, dout = inputs(case, bf16)
    name, B, H, T, L, spec, scale, rate, kind = case
    kp, c = case_keep(case) if isinstance(keep, str) else keep
    return Ref(q, k, v, dout, B, H, T, L, spec, scale, kp, c, mut=mut, device=device, unit=U16 if bf16 else U32)
