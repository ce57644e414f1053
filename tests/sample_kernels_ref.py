"""References for the sampling kernel (csrc/sample_rows.hip): the float64 reference of the six steps of include/vf_hip.h's contract
(temperature, top-k, top-p, counter-based Gumbel noise, the draw, its log-probability) with the decision margins the rounded class
needs; the float32 restatement of the kernel in its own order of operations, with the usual mistakes as mutants; the comparison
(``judge``) that the host and the GPU tests share; the inputs and case lists of tests/test_hip_sample.py.  tests/test_sample_ref_host.py
pins all of it on the CPU.

Classes.  Exact: the kept set and its threshold without top-p (a threshold on values, no rounding involved); membership of every draw in
the reference's kept set; top_k = 1.  Rounded, each with an exemption that is a statement about the float64 REFERENCE, never about the
kernel:
    idx    equals the reference's unless the float64 gap between the two largest y + g over the kept set is below
           c_key x 2^-24 x (max |y| + max |g|), both maxima over the kept set, and above 0: an exact tie (equal logits under equal noise
           words: ``tie_rows``) is decided by the lowest-index rule, exactly;
    kept / thr under top-p equal the reference's unless the float64 normalised mass at v* or at the next higher value lies within
           c_mass x 2^-24 of top_p (such a row's draws are exempt with it: they are drawn from another set);
    logp   within c_logp x 2^-24 x (|y_idx| + magnitude of lse) wherever idx and kept agree; magnitude of lse = |m| + |log s| +
           sum_kept p_n (1 + |y_n - m|), as tests/score_kernels_ref.py forms it.
At most CAP = 0.5 % of the (row, sample) cases of one test may be exempt."""
import math

import numpy as np
import torch

from training_kernels_ref import U, rng  # noqa: F401  (one definition of each, shared)

F32, F64, U64 = np.float32, np.float64, np.uint64
SITE_SAMPLE = 0x5A0000
CAP = 0.005
_M = U64(0xFFFFFFFF)


# ------------------------------------------------------------------ the noise, restated on its own (not through viewformer_amd/_hash.py)
def _mix(seed, site, idx):
    """vf_dropout_hash(seed, site, idx) of csrc/vf_common.h on uint64 arrays (site and idx broadcast)"""
    site, idx = np.asarray(site, dtype=U64), np.asarray(idx, dtype=U64)
    h = (U64(int(seed) & 0xFFFFFFFF) ^ ((site * U64(0x9E3779B9)) & _M)) & _M
    h = h ^ (idx & _M)
    h = (h * U64(0x85EBCA6B)) & _M
    h = h ^ (h >> U64(13))
    h = (h + (((idx >> U64(32)) * U64(0xC2B2AE35)) & _M) + U64(0x27D4EB2F)) & _M
    h = h ^ (h >> U64(16))
    h = (h * U64(0x165667B1)) & _M
    h = h ^ (h >> U64(15))
    h = (h * U64(0xD3A2646C)) & _M
    return h ^ (h >> U64(16))


def _lowbias(x):
    x = np.asarray(x, dtype=U64) & _M
    x = x ^ (x >> U64(16))
    x = (x * U64(0x7FEB352D)) & _M
    x = x ^ (x >> U64(15))
    x = (x * U64(0x846CA68B)) & _M
    return x ^ (x >> U64(16))


def uniform(seed, row_ids, S, N, keyed_by_s=True):
    """u [rows][S][N] float64 holding the exact fp32 values ((w >> 9) + 0.5) 2^-23, w = lowbias32(n ^ hash(seed, SITE_SAMPLE + s, row_id))"""
    rid = np.asarray(row_ids, dtype=np.int64).astype(U64).reshape(-1, 1)
    s = np.arange(S, dtype=U64).reshape(1, -1)
    key = _mix(seed, U64(SITE_SAMPLE) + (s if keyed_by_s else s * U64(0)), rid)                 # [rows][S]
    w = _lowbias(np.arange(N, dtype=U64).reshape(1, 1, -1) ^ key[:, :, None])
    return ((w >> U64(9)).astype(F64) + 0.5) * 2.0 ** -23


def gumbel64(u):
    return -np.log(-np.log1p(-(1.0 - u)))


def gumbel32(u):
    """the kernel's statements in float32: a = 1 - u (exact), -log1p(-a), -log"""
    a = (F32(1.0) - u.astype(F32)).astype(F32)
    return (-np.log((-np.log1p(-a)).astype(F32))).astype(F32)


# ------------------------------------------------------------------ the float64 reference
def _first_argmax(keys):
    mx = keys.max(-1, keepdims=True)
    n = keys.shape[-1]
    return np.where(keys == mx, np.arange(n), n).min(-1)


def sample_ref(z, temperature=1.0, top_k=0, top_p=1.0, seed=0, row_ids=None, S=1):
    """z [rows][N] float32 -> dict of numpy arrays:
    idx int64 [rows][S] (-1: no finite logit), logp float64 [rows][S], kept int32 [rows], thr float64 [rows] (NaN: no finite logit),
    keep bool [rows][N], gap float64 [rows][S] (between the two largest y + g over the kept set; inf where one code is kept), scale
    [rows][S] (max |y| + max |g| over the kept set), mass_at / mass_above float64 [rows] (normalised mass at v* and at the next higher
    value; NaN without top-p), logp_mag [rows][S]."""
    z = np.asarray(z, dtype=F32).astype(F64)
    rows, N = z.shape
    T, p = float(F32(temperature)), float(F32(top_p))
    row_ids = np.arange(rows) if row_ids is None else np.asarray(row_ids)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        y = z / T
        finite = y > -math.inf
        nf = finite.sum(1)
        empty = nf == 0
        srt = -np.sort(-y, 1)                                                        # descending
        keep = finite.copy()
        if top_k > 0:
            vk = srt[:, min(top_k, N) - 1]
            keep = np.where(((top_k < nf) & ~empty)[:, None], y >= vk[:, None], keep)
        m = np.where(empty, 0.0, y.max(1))
        e = np.where(keep, np.exp(y - m[:, None]), 0.0)
        mass_at, mass_above = np.full(rows, math.nan), np.full(rows, math.nan)
        if p < 1.0:
            order = np.argsort(-y, 1, kind='stable')
            ys, es = np.take_along_axis(y, order, 1), np.take_along_axis(e, order, 1)
            cs = np.cumsum(es, 1)
            total = cs[:, -1]
            for r in range(rows):
                if empty[r]:
                    continue
                i0 = int(np.argmax(cs[r] >= p * total[r]))                          # the smallest prefix whose mass reaches p ...
                v = ys[r, i0]
                keep[r] &= y[r] >= v                                                # ... with the ties at its last value
                mass_at[r] = es[r][ys[r] >= v].sum() / total[r]
                if v < ys[r, 0]:                                                    # (NaN where v* is the row's maximum: nothing is higher)
                    mass_above[r] = es[r][ys[r] > v].sum() / total[r]
            e = np.where(keep, e, 0.0)
        kept = keep.sum(1).astype(np.int32)
        thr = np.where(empty, math.nan, np.where(keep, y, math.inf).min(1))
        s_ = e.sum(1)
        ls = np.log(s_)
        prob = e / s_[:, None]
        dabs = np.where(keep, np.abs(y - m[:, None]), 0.0)
        lse_mag = np.abs(m) + np.abs(ls) + (prob * (1.0 + dabs)).sum(1)
        g = gumbel64(uniform(seed, row_ids, S, N))                                   # [rows][S][N]
        keys = np.where(keep[:, None, :], y[:, None, :] + g, -math.inf)
        idx = _first_argmax(keys)
        top2 = -np.sort(-keys, -1)[..., :2] if N > 1 else np.concatenate([keys, np.full_like(keys, -math.inf)], -1)
        gap = top2[..., 0] - top2[..., 1]
        ymax = np.where(keep, np.abs(y), 0.0).max(1)
        gmax = np.where(keep[:, None, :], np.abs(g), 0.0).max(-1)
        yi = np.take_along_axis(y, np.clip(idx, 0, N - 1), 1)
        logp = yi - (m + ls)[:, None]
        logp_mag = np.abs(yi) + lse_mag[:, None]
    idx = np.where(empty[:, None], -1, idx).astype(np.int64)
    logp = np.where(empty[:, None], math.nan, logp)
    return dict(idx=idx, logp=logp, kept=kept, thr=thr, keep=keep, gap=gap, scale=ymax[:, None] + gmax, mass_at=mass_at,
                mass_above=mass_above, logp_mag=logp_mag, empty=empty)


# ------------------------------------------------------------------ the float32 restatement of the kernel
def _img(z32):
    b = z32.view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)


def _exp_neg32(d):
    """vf_exp_neg behind the kernel's clamp: 0 below -88, results below the normal range flush to 0"""
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        e = np.exp(np.maximum(d.astype(F64), -200.0))
    e = np.where((d >= F32(-88.0)) & (e >= 2.0 ** -126), e, 0.0)
    return e.astype(F32)


def _mass32(e, mask):
    """sum of e where mask in the kernel's order: lane c % 64 adds its slots c // 64 ascending, then the xor butterfly 32 .. 1"""
    rows, N = e.shape
    slots = -(-N // 64)
    v = np.zeros((rows, slots * 64), F32)
    v[:, :N] = np.where(mask, e, F32(0))
    v = v.reshape(rows, slots, 64)
    part = np.zeros((rows, 64), F32)
    for j in range(slots):
        part = (part + v[:, j]).astype(F32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = (part + part[:, lanes ^ o]).astype(F32)
    return part[:, 0]


def _search(pred):
    """the largest 32-bit t with pred(t) true, from the top bit down (pred is monotone: true at 0): int64 [rows]"""
    t = None
    for bit in range(31, -1, -1):
        cand = (0 if t is None else t) | (1 << bit)
        ok = pred(cand)
        t = np.where(ok, cand, 0 if t is None else t)
    return t


MISTAKES = ('p_before_k', 'strict', 'temperature_last', 'logp_unfiltered', 'no_s', 'row_position', 'tie_high')


def sample_f32(z, temperature=1.0, top_k=0, top_p=1.0, seed=0, row_ids=None, S=1, mistake=None):
    """the kernel in float32, in its order: d = (z - max z) / T, e = e^d once per row; thresholds by bitwise search on the integer image of
    z (top-k: masked counts; top-p: masked masses against fl(top_p x mass)); keys d + g with g from 1 - u; logp = d_idx - log(mass).
    Returns idx, logp (float32), kept, thr (float32) and the per-code float32 keys d + g [rows][S][N] (for the calibration).
    ``mistake`` (what the host test must see rejected): one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    z = np.asarray(z, dtype=F32) + F32(0)
    rows, N = z.shape
    T, p = F32(temperature), F32(top_p)
    row_ids = np.arange(rows) if row_ids is None else np.asarray(row_ids)
    if mistake == 'row_position':
        row_ids = np.arange(rows)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore', under='ignore'):
        zmax = z.max(1)
        empty = zmax == -np.inf
        zm = np.where(empty, F32(0), zmax)
        Td = F32(1) if mistake == 'temperature_last' else T                        # the filters see z, the keys z / T
        d = ((z - zm[:, None]).astype(F32) / Td).astype(F32)
        e = _exp_neg32(d)
        k = _img(z)
        fin = k > 0x007FFFFF
        nf = fin.sum(1)
        kmin = np.where(fin, k, 0xFFFFFFFF).min(1)
        kmax = _img(zm)

        def topk(mask_in):
            if top_k <= 0:
                return kmin
            tk = _search(lambda c: (mask_in & (k >= np.reshape(c, (-1, 1)))).sum(1) >= top_k)
            return np.where(top_k < nf, tk, kmin)

        def topp(tk):
            if not p < 1:
                return tk
            base = k >= tk[:, None]
            target = (p * _mass32(e, base)).astype(F32)
            tp = _search(lambda c: _mass32(e, base & (k >= np.reshape(c, (-1, 1)))) >= target)
            return np.maximum(np.minimum(tp, kmax), tk)
        if mistake == 'p_before_k':
            tp = topp(kmin)
            t = np.maximum(topk(fin), tp)
        else:
            t = topp(topk(fin))
        keep = (k > t[:, None]) if mistake == 'strict' else (k >= t[:, None])
        keep &= fin
        if mistake == 'strict':
            keep |= (k == kmax[:, None]) & fin & (keep.sum(1) == 0)[:, None]
        mass = _mass32(e, keep)
        lsum = np.log(_mass32(e, fin) if mistake == 'logp_unfiltered' else mass).astype(F32)
        kept = keep.sum(1).astype(np.int32)
        thr = (np.where(keep, z, F32(np.inf)).min(1) / T).astype(F32)
        if mistake == 'temperature_last':
            d = ((z - zm[:, None]).astype(F32) / T).astype(F32)
        g = gumbel32(uniform(seed, row_ids, S, N, keyed_by_s=mistake != 'no_s'))
        keys = np.where(keep[:, None, :], (d[:, None, :] + g).astype(F32), F32(-np.inf))
        if mistake == 'tie_high':
            idx = N - 1 - _first_argmax(keys[..., ::-1])
        else:
            idx = _first_argmax(keys)
        di = np.take_along_axis(d, np.clip(idx, 0, N - 1), 1)
        logp = (di - lsum[:, None]).astype(F32)
    idx = np.where(empty[:, None], -1, idx).astype(np.int64)
    logp = np.where(empty[:, None], F32(np.nan), logp).astype(F32)
    return dict(idx=idx, logp=logp, kept=np.where(empty, 0, kept).astype(np.int32), thr=np.where(empty, F32(np.nan), thr).astype(F32),
                keys=keys, d=d, e=e, keep=keep, zmax=zm)


# ------------------------------------------------------------------ the comparison
def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def judge(got, ref, top_p, c_key, c_mass, c_logp):
    """got: dict with idx [rows][S] and any of logp, kept, thr (tensors or arrays); ref: sample_ref's.  Returns dict(cases, exempt,
    errors [str], worst_logp (in units of 2^-24 x magnitude)).  The caller asserts errors == [] and exempt <= CAP x cases."""
    idx = _np(got['idx']).astype(np.int64)
    rows, S = idx.shape
    N = ref['keep'].shape[1]
    errors = []
    empty = ref['empty']
    live = ~empty
    # rows without a distribution
    if not np.array_equal(idx[empty], ref['idx'][empty]):
        errors.append('idx of a row without a finite logit is not -1')
    # the kept set
    row_exempt = np.zeros(rows, bool)
    if float(F32(top_p)) < 1.0:
        with np.errstate(invalid='ignore'):
            near = (np.abs(ref['mass_at'] - float(F32(top_p))) <= c_mass * U) | (np.abs(ref['mass_above'] - float(F32(top_p))) <= c_mass * U)
        row_exempt = near & live
    kept_ok = np.ones(rows, bool)
    if 'kept' in got:
        kept_ok = _np(got['kept']).astype(np.int64) == ref['kept']
        bad = ~kept_ok & ~row_exempt
        if bad.any():
            errors.append(f'kept differs in {int(bad.sum())} rows, first row {int(np.argmax(bad))}: {_np(got["kept"])[bad][:4]} vs {ref["kept"][bad][:4]}')
    if 'thr' in got:
        t = _np(got['thr']).astype(F64)
        same = (t == ref['thr'].astype(F32).astype(F64)) | (np.isnan(t) & np.isnan(ref['thr']))
        kept_ok = kept_ok & same
        bad = ~same & ~row_exempt
        if bad.any():
            errors.append(f'thr differs in {int(bad.sum())} rows, first row {int(np.argmax(bad))}')
    # membership: no exemption
    member = np.take_along_axis(ref['keep'], np.clip(idx, 0, N - 1), 1) & (idx >= 0) & (idx < N)
    if not member[live].all():
        errors.append(f'{int((~member[live]).sum())} draws are outside the reference\'s kept set')
    # the draw
    # an EXACT float64 tie (gap 0) is no rounding matter: it comes from equal logits under equal noise words, whose float32 keys are equal
    # bit for bit as well, so the rule "on equal keys the lowest index wins" applies as it stands and nothing is exempt
    case_exempt = ((ref['gap'] < c_key * U * ref['scale']) & (ref['gap'] > 0)) | row_exempt[:, None]
    case_exempt &= live[:, None]
    same_idx = idx == ref['idx']
    bad = ~same_idx & ~case_exempt
    if bad.any():
        r, s = np.argwhere(bad)[0]
        errors.append(f'idx differs in {int(bad.sum())} cases outside the exemption, first (row {r}, s {s}): {idx[r, s]} vs {ref["idx"][r, s]}, '
                      f'gap {ref["gap"][r, s]:.3e}, scale {ref["scale"][r, s]:.3e}')
    worst = 0.0
    if 'logp' in got:
        lp = _np(got['logp']).astype(F64)
        if not np.isnan(lp[empty]).all():
            errors.append('logp of a row without a finite logit is not NaN')
        sel = same_idx & kept_ok[:, None] & live[:, None]
        if sel.any():
            with np.errstate(invalid='ignore', divide='ignore'):
                err, mag = np.abs(lp - ref['logp'])[sel], (U * ref['logp_mag'])[sel]
                ratio = np.where(mag > 0, err / mag, np.where(err == 0, 0.0, math.inf))
            ratio = np.where(np.isfinite(lp[sel]), ratio, math.inf)
            worst = float(ratio.max())
            if not worst <= c_logp:
                errors.append(f'logp: {worst:.3f} x 2^-24 x magnitude exceeds c = {c_logp:g}')
    return dict(cases=int(live.sum()) * S, exempt=int(case_exempt.sum()), errors=errors, worst_logp=worst)


def deviations(z, ref, r32, top_p):
    """what the constants are calibrated on: the float32 restatement's worst deviation from the float64 reference, in the units of the
    three tolerances: (key, mass, logp).
    key:  |(d + g)_32 - ((y + g)_64 - max y)| over the codes both keep, / (2^-24 x (max |y| + max |g|)), in rows that keep two codes or more;
    mass: |r32(v) - r64(v)| / 2^-24 at every value v of the row that top-k left, r64 = normalised mass at v, r32 = mass32(v) x top_p /
          fl(top_p x total32): the kernel keeps v's prefix iff r32 >= top_p, the reference iff r64 >= top_p;
    logp: |logp32 - logp64| / (2^-24 x magnitude) where idx and kept agree."""
    z64 = np.asarray(z, dtype=F32).astype(F64)
    T, p = float(F32(r32['T'])), float(F32(top_p))
    rows, N = z64.shape
    live = ~ref['empty']
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        y = z64 / T
        m = np.where(live, np.where(np.isfinite(y), y, -math.inf).max(1), 0.0)
        both = ref['keep'] & r32['keep']
        S = r32['keys'].shape[1]
        g64 = r32['g64']
        k64 = y[:, None, :] + g64 - m[:, None, None]
        dev = np.where(both[:, None, :], np.abs(r32['keys'].astype(F64) - k64), 0.0).max(-1)
        decided = live & (ref['kept'] >= 2)                                         # one kept code: nothing to decide, the gap is infinite
        key = float((dev / (U * ref['scale']))[decided].max()) if decided.any() else 0.0
        mass = 0.0
        if p < 1.0:
            base32, base64 = r32['base'], ref['base']
            e64 = np.where(base64, np.exp(y - m[:, None]), 0.0)
            tot64 = e64.sum(1)
            tot32 = _mass32(r32['e'], base32)
            tgt32 = (F32(top_p) * tot32).astype(F32).astype(F64)
            for r in np.nonzero(live)[0]:
                vals = np.unique(y[r][base64[r] & base32[r]])
                if vals.size > 48:                                                  # the values around the decision, and a spread of the others
                    ms = np.array([e64[r][y[r] >= v].sum() / tot64[r] for v in vals])
                    near = np.argsort(np.abs(ms - p))[:32]
                    vals = vals[np.unique(np.concatenate([near, np.linspace(0, vals.size - 1, 16).astype(int)]))]
                for v in vals:
                    r64 = e64[r][y[r] >= v].sum() / tot64[r]
                    m32 = float(_mass32(r32['e'][r:r + 1], (base32[r] & (y[r] >= v))[None])[0])
                    mass = max(mass, abs(m32 * p / tgt32[r] - r64) / U)
        sel = (r32['idx'] == ref['idx']) & (r32['kept'] == ref['kept'])[:, None] & live[:, None]
        logp = float((np.abs(r32['logp'].astype(F64) - ref['logp'])[sel] / (U * ref['logp_mag'])[sel]).max()) if sel.any() else 0.0
    return key, mass, logp


# ------------------------------------------------------------------ inputs and cases
KINDS = ('spread', 'flat', 'ascending', 'descending', 'all_equal', 'two_level', 'neg_inf_entries', 'all_neg_inf', 'normal4')
PAD = 4
ROWS = (1, 3, 65)
NS = (1, 63, 64, 65, 1024, 1026)
SS = (1, 3, 8)
TS = (0.5, 1.0, 2.0)
TOP_PS = (1.0, 0.9, 0.5, 1e-6)


def top_ks(N):
    return (0, 1, 2, 64, N, N + 5)


def two_level_positions(N):
    return sorted({0, N // 3, N // 2, N - 1})


def row_of(kind, N, g):
    if kind == 'spread':                                                            # normal, clipped to a +-60 spread
        return np.clip(g.standard_normal(N) * 20.0, -60.0, 60.0)
    if kind == 'flat':                                                              # nearly uniform
        return g.standard_normal(N) * 0.01
    if kind == 'ascending':
        return (np.arange(N) - N // 2) / 64.0
    if kind == 'descending':
        return (N // 2 - np.arange(N)) / 64.0
    if kind == 'all_equal':
        return np.full(N, 1.5)
    if kind == 'two_level':                                                         # 4 zeros (fewer for N < 4), the rest -100
        x = np.full(N, -100.0)
        x[two_level_positions(N)] = 0.0
        return x
    if kind == 'neg_inf_entries':
        x = g.standard_normal(N) * 3.0
        x[g.random(N) < 0.33] = -np.inf
        x[N // 2] = 1.0                                                             # the row keeps a finite code
        return x
    if kind == 'all_neg_inf':
        return np.full(N, -np.inf)
    if kind == 'normal4':
        return g.standard_normal(N) * 4.0
    raise KeyError(kind)


def inputs(rows, N, shift=0, seed=0):
    """([rows][N + PAD] float32 with +3e38 in the pad columns: a read past N wins the row; kinds [rows]; row_ids int64 [rows]).  Row r is
    of kind KINDS[(r + shift) % 9]; the row ids are 64-bit numbers with both halves in use."""
    g = rng(3000 + 11 * rows + N + 101 * shift + seed)
    kinds = [KINDS[(r + shift) % len(KINDS)] for r in range(rows)]
    x = np.empty((rows, N + PAD), F32)
    for r, kind in enumerate(kinds):
        x[r, :N] = row_of(kind, N, g).astype(F32)
    x[:, N:] = 3e38
    row_ids = (np.arange(rows, dtype=np.int64) % 3 << 32) | (np.arange(rows, dtype=np.int64) * 64 + 7 * shift)
    return torch.from_numpy(x), kinds, torch.from_numpy(row_ids)


def cases(N):
    """every (top_k, top_p) pair of the issue's lists at this N; rows, S, T, the layout, the seed and the kinds' shift walk their lists
    with the case number, so that every value of every dimension meets every N:
    (rows, N, S, T, top_k, top_p, padded, seed, shift)"""
    out = []
    i = NS.index(N)
    for ki, top_k in enumerate(top_ks(N)):
        for pi, top_p in enumerate(TOP_PS):                                        # (the layout alternates with top_k AND top_p: at every N each meets both)
            out.append((ROWS[i % 3], N, SS[(i // 3) % 3], TS[(i // 2) % 3], top_k, top_p, bool((ki + pi) % 2),
                        11 + i % 5, i % len(KINDS)))
            i += 1
    return out


def all_cases():
    return [c for N in NS for c in cases(N)]


def reference_for(case):
    rows, N, S, T, top_k, top_p, padded, seed, shift = case
    x, kinds, row_ids = inputs(rows, N, shift)
    return x, kinds, row_ids, sample_ref(x[:, :N].numpy(), T, top_k, top_p, seed, row_ids.numpy(), S)


def restatement_for(case, x, row_ids, ref, mistake=None):
    """sample_f32 on the case, with what ``deviations`` needs beside it"""
    rows, N, S, T, top_k, top_p, padded, seed, shift = case
    z = x[:, :N].numpy()
    r32 = sample_f32(z, T, top_k, top_p, seed, row_ids.numpy(), S, mistake=mistake)
    r32['T'] = T
    r32['g64'] = gumbel64(uniform(seed, row_ids.numpy(), S, N))
    nokp32 = sample_f32(z, T, top_k, 1.0, seed, row_ids.numpy(), 1)
    r32['base'] = nokp32['keep']
    ref['base'] = sample_ref(z, T, top_k, 1.0, seed, row_ids.numpy(), 1)['keep']
    return r32


def tie_rows(N, seed=21, others=-40.0, want=4):
    """Rows whose two best keys tie EXACTLY, in float64 and bit for bit in any float32 evaluation: two codes n1 < n2 that draw the same
    23-bit noise word ((w >> 9) equal, found by search over row ids x 64 samples) hold the same logit 0, every other code holds
    ``others`` (kept, but -40 + 16.7 < 0 - 2.8: it cannot win).  Returns (z [rows][N] float32, row_ids int64 [rows], picks [(s, n1, n2)]),
    S = 64: sample s of row r must be n1.  Up to ``want`` pairs in different lanes (n1 % 64 != n2 % 64: decided by the kernel's butterfly)
    and any pair in one lane (n2 - n1 a multiple of 64: decided by the lane's strict compare) that the search meets on its way — none so
    far: among some 1400 colliding pairs of 32 768 streams no two codes 64 k apart shared a noise word, so the in-lane half of the rule
    is not reached by an exact tie."""
    cross, same = [], []
    for block in range(8):                                                          # 64 row ids x 64 samples at a time, until both kinds are found
        rids = np.arange(64, dtype=np.int64) + 1000 + 64 * block + (np.int64(5) << 32)
        u = uniform(seed, rids, 64, N)
        us = np.sort(u, -1)
        ndup = (us[..., 1:] == us[..., :-1]).sum(-1)
        for r, s in np.argwhere(ndup == 1):                                         # exactly one pair, so the winner is one of the two
            order = np.argsort(u[r, s], kind='stable')
            j = int(np.argmax(us[r, s][1:] == us[r, s][:-1]))
            n1, n2 = sorted((int(order[j]), int(order[j + 1])))
            (same if (n2 - n1) % 64 == 0 else cross).append((int(rids[r]), int(s), n1, n2))
        if len(cross) >= want:
            break
    chosen = cross[:want] + same[:want]
    z = np.full((len(chosen), N), others, F32)
    for i, (_, s, n1, n2) in enumerate(chosen):
        z[i, n1] = z[i, n2] = 0.0
    return z, np.array([c[0] for c in chosen], dtype=np.int64), [c[1:] for c in chosen]


def in_order_sum(x):
    """[views][L] float32 tensor -> the sequential float32 sum over L"""
    s = x[:, 0].clone()
    for l in range(1, x.shape[1]):
        s = s + x[:, l]
    return s
