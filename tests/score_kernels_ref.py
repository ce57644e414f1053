"""References for the scoring kernels (csrc/lmhead_score.hip): the five per-row statistics of a row of logits z — first arg-max, its
logit, the logit of a target code, log-sum-exp, entropy — in float64, each as (value, magnitude); float32 restatements of both kernels'
formulas (the fused head's online rescaling merge in the kernel's order, the row kernel's two passes); the input generators and case
lists of tests/test_hip_score.py.  tests/test_score_ref_host.py pins all of it on the CPU.

Magnitudes (rounded class: |got - want| <= c x 2^-24 x magnitude) are the reference expression with every summand replaced by its
absolute value, formed where the value is formed:
    lse     = max + log s,  s = sum_n e^(z_n - max)            magnitude |max| + |log s| + sum_n p_n (1 + |z_n - max|)
    entropy = lse - sum_n p_n z_n,  p_n = e^(z_n - lse)        magnitude of lse + sum_n p_n |z_n| (1 + |z_n - max|)
An exponential is judged against p (1 + |z - max|): its argument z - max carries a rounding of that size, which the exponential turns
into a relative error (as the softmax references of tests/transformer_kernels_ref.py do).  A code of probability 0 (z = -inf) adds
nothing.  idx, max_logit and target_logit are selections: exact class, no magnitude."""
import math

import numpy as np
import torch

from training_kernels_ref import U, F64, t64, rng, normal, mismatches, worst_ratio, rejects  # noqa: F401  (one definition of each, shared)

F32 = np.float32
OUTPUTS = ('idx', 'max_logit', 'lse', 'target_logit', 'entropy')


# ------------------------------------------------------------------ float64 references
def score_stats(z, target=None):
    """z [rows][N] -> dict name -> (value, magnitude or None).  A row of nothing but -inf: idx 0, max = lse = -inf, entropy NaN.
    target outside [0, N): target_logit -inf."""
    z = t64(z)
    rows, N = z.shape
    mx = z.max(1).values
    col = torch.arange(N, device=z.device)
    idx = torch.where(z == mx[:, None], col, N).min(1).values
    empty = mx == -math.inf
    d = torch.where(empty[:, None], torch.zeros_like(z), z - mx[:, None])             # z - max, <= 0 (-inf for a code of probability 0)
    e = torch.where(empty[:, None], torch.zeros_like(z), torch.exp(d))
    s = e.sum(1)
    ls = torch.log(s)
    p = e / s[:, None]
    live = e > 0
    dz = torch.where(live, d, torch.zeros_like(d))
    zz = torch.where(live, z, torch.zeros_like(z))
    lse = torch.where(empty, mx, mx + ls)
    lse_mag = mx.abs() + ls.abs() + (p * (1.0 + dz.abs())).sum(1)                   # formed beside lse = max + log s
    ent = lse - (p * zz).sum(1)
    ent_mag = lse_mag + (p * zz.abs() * (1.0 + dz.abs())).sum(1)                    # formed beside entropy = lse - sum p z
    nan = torch.full_like(ent, math.nan)
    out = dict(idx=(idx, None), max_logit=(mx, None), lse=(lse, torch.where(empty, nan, lse_mag)),
               entropy=(torch.where(empty, nan, ent), torch.where(empty, nan, ent_mag)))
    if target is not None:
        t = torch.as_tensor(target).long().to(z.device)
        ok = (t >= 0) & (t < N)
        out['target_logit'] = (torch.where(ok, z.gather(1, t.clamp(0, N - 1)[:, None])[:, 0], torch.full_like(mx, -math.inf)), None)
    return out


def token_log_prob(z, target):
    """log p(target) = target_logit - lse, magnitude |target_logit| + magnitude of lse"""
    st = score_stats(z, target)
    return st['target_logit'][0] - st['lse'][0], st['target_logit'][0].abs() + st['lse'][1]


# ------------------------------------------------------------------ float32 restatements
def _merge32(a, b, mistake=None):
    """(m, i, s, t) absorbs (om, oi, os, ot), float32, as csrc/lmhead_score.hip's merge(): the side with the lower maximum is rescaled
    by e^d, d = -|m - om|:  s <- s e^d,  t <- (t + d s) e^d"""
    m, i, s, t = a
    om, oi, os_, ot = b
    with np.errstate(invalid='ignore', over='ignore'):
        d = -np.abs(m - om).astype(F32)
        e = np.exp(d).astype(F32) if mistake != 'no_rescale' else np.ones_like(d)
        dd = d if mistake != 'no_rescale' else np.zeros_like(d)
        ow = om > m
        ls, lt = np.where(ow, s, os_), np.where(ow, t, ot)
        hs, ht = np.where(ow, os_, s), np.where(ow, ot, t)
        s2 = (hs + (ls * e).astype(F32)).astype(F32)
        t2 = (ht + ((lt + (dd * ls).astype(F32)).astype(F32) * e).astype(F32)).astype(F32)
        take = ow | ((om == m) & ((oi < i) if mistake != 'tie_high' else (oi > i)))
    return np.where(take, om, m), np.where(take, oi, i), s2, t2


def fused_score_f32(z, target=None, mistake=None):
    """the fused kernel's epilogue on float32 logits z [rows][N], N % 128 == 0, in its order: wave w (of 4) owns codes [w N/4, (w+1) N/4),
    lane l of 32 walks codes w N/4 + 32 nt + l ascending with an online (max, first index, s, t); then the xor butterfly 16, 8, 4, 2, 1
    over the lanes, then waves 0..3.  lse = max + log s, entropy = log s - t / s.  ``mistake`` (what the host test must see rejected):
    'no_rescale', 'drop_tile' (a wave's last tile never merged), 'entropy_sign', 'tie_high', 'wrong_row' (the target's logit taken as if
    accumulator row r were tile row r: the MFMA layout's row (r & 3) + 8 (r >> 2) + 4 half ignored)."""
    z = np.asarray(z, dtype=F32)
    rows, N = z.shape
    assert N % 128 == 0
    tiles = N // 128
    zz = z.reshape(rows, 4, tiles, 32)
    code = np.arange(N, dtype=np.int64).reshape(4, tiles, 32)
    m, i = zz[:, :, 0].copy(), np.broadcast_to(code[:, 0], (rows, 4, 32)).copy()
    s, t = np.ones_like(m), np.zeros_like(m)
    last = tiles - 1 if (mistake == 'drop_tile' and tiles > 1) else tiles
    for nt in range(1, last):
        one = (zz[:, :, nt], np.broadcast_to(code[:, nt], (rows, 4, 32)), np.ones_like(m), np.zeros_like(m))
        # the kernel's in-lane update is merge() with the newcomer's (z, 1, 0); a tie keeps the earlier code
        m, i, s, t = _merge32((m, i, s, t), one, mistake)
    lanes = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        part = lanes ^ o
        m, i, s, t = _merge32((m, i, s, t), (m[..., part], i[..., part], s[..., part], t[..., part]), mistake)
    st = (m[:, 0, 0], i[:, 0, 0], s[:, 0, 0], t[:, 0, 0])
    for w in range(1, 4 if not (mistake == 'drop_tile' and tiles == 1) else 3):
        st = _merge32(st, (m[:, w, 0], i[:, w, 0], s[:, w, 0], t[:, w, 0]), mistake)
    m, i, s, t = st
    ls = np.log(s).astype(F32)
    ent = (ls - (t / s).astype(F32)).astype(F32)
    out = dict(idx=i.astype(np.int64), max_logit=m, lse=(m + ls).astype(F32), entropy=-ent if mistake == 'entropy_sign' else ent)
    if target is not None:
        tg = np.asarray(target).astype(np.int64)
        ok = (tg >= 0) & (tg < N)
        r = np.arange(rows)
        if mistake == 'wrong_row':
            rl = r % 32
            acc_r, half = rl % 16, rl // 16                               # read accumulator row r of half-wave `half` as tile row 16 half + r
            r = r - rl + np.minimum((acc_r & 3) + 8 * (acc_r >> 2) + 4 * half, 31)
            r = np.minimum(r, rows - 1)
        out['target_logit'] = np.where(ok, z[r, np.clip(tg, 0, N - 1)], F32(-np.inf)).astype(F32)
    return out


def rows_score_f32(z, target=None):
    """the row kernel's two passes on float32 logits z [rows][N]: max / first index; then 64 lane-strided partial sums of e^(z - max) and
    (z - max) e^(z - max) (0 where the exponential is 0) and the xor butterfly 32 .. 1 over them"""
    z = np.asarray(z, dtype=F32)
    rows, N = z.shape
    m = z.max(1)
    idx = np.where(z == m[:, None], np.arange(N), N).min(1)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        d = (z - m[:, None]).astype(F32)
        e = np.exp(d).astype(F32)
        te = np.where(e > 0, (d * e).astype(F32), F32(0))
        ps, pt = np.zeros((rows, 64), F32), np.zeros((rows, 64), F32)
        for c0 in range(0, N, 64):
            w = min(64, N - c0)
            ps[:, :w] = (ps[:, :w] + e[:, c0:c0 + w]).astype(F32)
            pt[:, :w] = (pt[:, :w] + te[:, c0:c0 + w]).astype(F32)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            ps, pt = (ps + ps[:, lanes ^ o]).astype(F32), (pt + pt[:, lanes ^ o]).astype(F32)
        s, t = ps[:, 0], pt[:, 0]
        ls = np.log(s).astype(F32)
        empty = m == -np.inf
        out = dict(idx=idx.astype(np.int64), max_logit=m, lse=np.where(empty, F32(-np.inf), (m + ls).astype(F32)),
                   entropy=np.where(empty, F32(np.nan), (ls - (t / s).astype(F32)).astype(F32)))
    if target is not None:
        tg = np.asarray(target).astype(np.int64)
        ok = (tg >= 0) & (tg < N)
        out['target_logit'] = np.where(ok, z[np.arange(rows), np.clip(tg, 0, N - 1)], F32(-np.inf)).astype(F32)
    return out


# ------------------------------------------------------------------ inputs: the fused kernel
FUSED_M = (1, 31, 32, 33, 65)
FUSED_KN = ((128, 128), (128, 1024), (768, 1024))       # N = 128: each wave has exactly one tile
FUSED_KINDS = ('normal', 'spread', 'ascending', 'descending', 'tie_lanes', 'tie_waves', 'tie_tiles', 'max_last', 'flat')
LDH_PAD = 8                                             # padded ldh: a multiple of 8 elements serves fp32 and bf16 rows


def bf16_round(a):
    return torch.as_tensor(a, dtype=torch.float32).to(torch.bfloat16).to(torch.float32)


def fused_inputs(M, K, N):
    """(h [M][K] fp32, wte [N][K] fp32, target int32 [M], kinds [M]).  Row m is of kind FUSED_KINDS[m % 9]:
    'normal'      random h: logits of std ~3
    every other kind has h[m] = e_k (one 1.0, exact in bf16) so that z[m][n] = bf16(wte[n][k]) EXACTLY, column k of wte being
    'spread'      a ramp over +-60 in random order: the tails underflow against the maximum
    'ascending'   strictly increasing in n over 2^-4 .. 2^4, maximum at N - 1 (last tile of the last wave): every lane's maximum moves
                  at every tile
    'descending'  the same reversed, maximum at 0 (first tile of wave 0): no lane's maximum moves, every merge rescales the other side
    'tie_lanes'   the maximum 9 at codes 3 and 4 (neighbouring lanes)         'tie_waves'  at 7 and 7 + N/4 (two waves, one lane)
    'tie_tiles'   at 5 and 37 (one lane, two tiles; N = 128: lanes 5 and 6)   'max_last'   a lone maximum at N - 1 over noise
    'flat'        noise of std 0.05: a nearly uniform distribution, what an untrained model gives — max ~ 0, lse ~ entropy ~ log N, so
                  that the roundings of log s and of the last subtraction are not hidden behind a large |max| in the magnitude
    Targets walk 0, 31, 32, N/4 - 1, N/4, N - 1, -1, N, then the row's arg-max or a random code."""
    g = rng(1000 + 7 * M + K + N)
    wte = (g.standard_normal((N, K)) * (3.0 / math.sqrt(K))).astype(np.float32)
    h = g.standard_normal((M, K)).astype(np.float32)
    n = np.arange(N, dtype=np.float64)
    # N consecutive (N = 128: every eighth) bf16 numbers from 2^-4 up to 2^4: strictly increasing and exact in bf16
    ramp = (torch.arange(N, dtype=torch.int32) * (1024 // N) + 0x3D80).to(torch.int16).view(torch.bfloat16).double().numpy()
    cols = {
        'spread': g.permutation(N) / (N - 1.0) * 120.0 - 60.0,
        'ascending': ramp,
        'descending': ramp[::-1].copy(),
        'tie_lanes': np.where((n == 3) | (n == 4), 9.0, g.standard_normal(N)),
        'tie_waves': np.where((n == 7) | (n == 7 + N // 4), 9.0, g.standard_normal(N)),
        'tie_tiles': np.where((n == 5) | (n == (37 if N >= 256 else 6)), 9.0, g.standard_normal(N)),
        'max_last': np.where(n == N - 1, 7.0, g.standard_normal(N)),
        'flat': g.standard_normal(N) * 0.05,
    }
    kinds = [FUSED_KINDS[m % len(FUSED_KINDS)] for m in range(M)]
    for j, kind in enumerate(FUSED_KINDS[1:]):
        wte[:, j] = cols[kind]
    wte = bf16_round(wte).numpy()
    for m, kind in enumerate(kinds):
        if kind != 'normal':
            h[m] = 0.0
            h[m, FUSED_KINDS.index(kind) - 1] = 1.0
    fixed = [0, 31, 32, N // 4 - 1, N // 4, N - 1, -1, N]
    target = np.array([fixed[m] if m < len(fixed) else int(g.integers(0, N)) for m in range(M)], dtype=np.int32)
    return torch.from_numpy(h), torch.from_numpy(wte), torch.from_numpy(target), kinds


def fused_logits_f32(h, wte):
    """float32 logits of the bf16-rounded operands (float64 products, one rounding): what the epilogue sees up to the accumulation order.
    Exact for the one-hot rows."""
    return (bf16_round(h).double() @ bf16_round(wte).double().t()).float()


# ------------------------------------------------------------------ inputs: the row kernel
ROWS_N = (1, 63, 64, 65, 1024, 1026)
ROWS_PAD = 4
ROWS_KINDS = ('normal', 'spread', 'ties', 'neg_inf_entries', 'all_neg_inf', 'flat')


def rows_inputs(rows, N, kind):
    """([rows][N + 4] fp32 with +3e38 in the four pad columns: a read past N wins the row; target int32 [rows]).  'spread': +-60;
    'ties': the maximum 9 at c and c + 1 and (N >= 65) c + 64; 'neg_inf_entries': a third of the codes -inf, the target's among them in
    row 0; 'all_neg_inf': row rows // 2 is nothing but -inf; 'flat': std 0.05, a nearly
    uniform distribution (an untrained model's), where nothing large in the magnitude hides the roundings of log s."""
    g = rng(2000 + 5 * rows + N + ROWS_KINDS.index(kind))
    x = (g.standard_normal((rows, N + ROWS_PAD)) * 3.0).astype(np.float32)
    target = g.integers(0, N, size=rows).astype(np.int32)
    if kind == 'spread':
        x[:, :N] = (g.random((rows, N)) * 120.0 - 60.0).astype(np.float32)
    elif kind == 'ties':
        for r in range(rows):
            c = (37 * r + N // 3) % N
            x[r, c] = 9.0
            x[r, min(c + 1, N - 1)] = 9.0
            if N >= 65:
                x[r, (c % (N - 64)) + 64] = 9.0
                x[r, c % (N - 64)] = 9.0
    elif kind == 'neg_inf_entries':
        x[:, :N][g.random((rows, N)) < 0.33] = -np.inf
        x[:, N // 2] = 1.0                                                       # every row keeps a finite code
        x[0, target[0]] = -np.inf if target[0] != N // 2 else 1.0
    elif kind == 'all_neg_inf':
        x[rows // 2, :N] = -np.inf
    elif kind == 'flat':                                                         # nearly uniform: max ~ 0, lse ~ entropy ~ log N
        x[:, :N] = (g.standard_normal((rows, N)) * 0.05).astype(np.float32)
    x[:, N:] = 3e38
    fixed = [0, N - 1, -1, N]
    for r in range(min(rows, len(fixed))):
        if not (kind == 'neg_inf_entries' and r == 0):
            target[r] = fixed[r]
    return torch.from_numpy(x), torch.from_numpy(target)


def split_special(got, want):
    """rounded class with non-finite reference values: (number of elements where NaN / +inf / -inf do not sit exactly where the reference
    has them, mask of the elements to judge by worst_ratio)"""
    got, want = t64(got), t64(want)
    fin = torch.isfinite(want)
    bad = (torch.isnan(got) != torch.isnan(want)) | ((got == math.inf) != (want == math.inf)) | ((got == -math.inf) != (want == -math.inf))
    return int(bad.sum()), fin
