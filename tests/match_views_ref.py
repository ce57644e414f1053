"""References for the many-to-many score (csrc/match_views.hip, vf_match_views_f32): P photos against M cameras per scene from the M
views' logits.  For every (b, m, p), with c_t = codes[b][p][t] and row_t = (b M + m) L + t:
    x_t = (0 <= c_t < V) ? logits[row_t][c_t] - lse[row_t] : -inf
    log_likelihood[b][m][p] = sum_t x_t          accuracy[b][m][p] = #{t : idx[row_t] == c_t} / L
``reference`` states it in float64 FROM the float32 logits and lse (value and the magnitude sum_t |z_t - lse_t|); ``restated_f32`` in
float32 in the kernel's order (one rounded subtraction per token, one chain of rounded additions in token order) — the GPU test asks for
its bits.  ``CASES`` / ``inputs`` are the case list and the inputs of tests/test_hip_match.py; tests/test_match_views_ref_host.py pins all
of it on the CPU, with the mistakes (``MISTAKES``) that the restatement must tell from the reference.

Rounded class: |got - want| <= gamma_L x magnitude, gamma_L = L u / (1 - L u), u = 2^-24: the textbook bound of a recursive sum of L terms
(L - 1 additions) plus the one rounding of each term's subtraction.  Derived, not calibrated.

NaN: -inf - -inf (an in-range code on a row of nothing but -inf) is a NaN whose sign and payload IEEE 754 leaves open (x86 produces
0xFFC00000, the GPU 0x7FC00000), so ``bits`` maps every NaN to one pattern before bits are compared; every other value keeps its own."""
import numpy as np
import torch

from training_kernels_ref import U, rng  # noqa: F401  (one definition of each, shared)

F32 = np.float32
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
PAD_FILL = 3e38                           # in the columns V..ld-1: a read past V dominates whatever it is added to
MISTAKES = ('pairwise', 'sum_then_sub', 'swap_pm', 'next_photo', 'clamp', 'ignore_stride', 'acc_over_V')

# (L, V, ld - V, B, M, P, scene stride: 'shared' = 0 / 'dense' = P L / 'gap' = P L + 3, logit spread): a pruned product in which every
# value the kernel can go wrong at appears — L below, at and above the 32-token slab and its multiple; V = 1 and a non-power of two; P
# below, at and above one wave, and above one 256-photo workgroup; every case has room for the six planted codes
CASES = [
    dict(L=1, V=1, pad=0, B=1, M=2, P=63, stride='dense', spread=0.05),
    dict(L=3, V=7, pad=5, B=3, M=2, P=65, stride='gap', spread=3.0),
    dict(L=64, V=128, pad=0, B=3, M=5, P=64, stride='shared', spread=60.0),
    dict(L=65, V=1024, pad=5, B=1, M=2, P=257, stride='shared', spread=3.0),
    dict(L=64, V=1024, pad=5, B=3, M=1, P=1, stride='dense', spread=60.0),
    dict(L=65, V=7, pad=0, B=3, M=5, P=257, stride='gap', spread=0.05),
    dict(L=3, V=128, pad=5, B=1, M=5, P=64, stride='dense', spread=60.0),
    dict(L=1, V=1024, pad=0, B=3, M=2, P=257, stride='gap', spread=3.0),
]


def case_id(c):
    return f"L{c['L']}-V{c['V']}-ld{c['V'] + c['pad']}-B{c['B']}-M{c['M']}-P{c['P']}-{c['stride']}-s{c['spread']:g}"


def gamma(L):
    return L * U / (1.0 - L * U)


def scene_stride(c):
    return {'shared': 0, 'dense': c['P'] * c['L'], 'gap': c['P'] * c['L'] + 3}[c['stride']]


def inputs(c, seed=0):
    """-> dict(logits fp32 [B M L][ld] (columns V.. = PAD_FILL), lse fp32 and idx int64 [B M L] (the float64 log-sum-exp of the row rounded
    once, the first arg-max), codes int32 [B or 1][P][L], inf_row).  One row (``inf_row``) is nothing but -inf: lse -inf, idx 0.  About a
    third of the codes are some camera's arg-max (accuracy has hits); six codes of every case are 0, V - 1, -1, V, INT32_MIN, INT32_MAX."""
    L, V, B, M, P = c['L'], c['V'], c['B'], c['M'], c['P']
    g = rng(1000 + 7 * seed + L + 3 * V + 5 * P + 11 * M + 13 * B)
    R, ld = B * M * L, V + c['pad']
    logits = np.full((R, ld), PAD_FILL, dtype=F32)
    logits[:, :V] = (g.standard_normal((R, V)) * c['spread']).astype(F32)
    inf_row = R // 2
    logits[inf_row, :V] = -np.inf
    z = logits[:, :V].astype(np.float64)
    mx = z.max(1)
    with np.errstate(invalid='ignore', divide='ignore'):
        lse = np.where(np.isinf(mx), -np.inf, mx + np.log(np.exp(z - np.where(np.isinf(mx), 0.0, mx)[:, None]).sum(1))).astype(F32)
    idx = z.argmax(1).astype(np.int64)                                   # numpy: the first maximum
    Bc = 1 if c['stride'] == 'shared' else B
    codes = g.integers(0, V, size=(Bc, P, L)).astype(np.int32)
    pred = idx.reshape(B, M, L)
    for b in range(Bc):
        for p in range(P):
            hit = g.random(L) < 0.33
            codes[b, p, hit] = pred[b, p % M, hit]
    # the planted codes: 0 and V - 1 in the first and the middle photo; the four out-of-range ones in the LAST photos (at most half of
    # them, so that photos with a finite log-likelihood remain), each at a token of its own
    ph = codes.reshape(Bc * P, L)
    n_ph = Bc * P
    nbad = max(1, min(4, n_ph // 2))
    assert n_ph >= 2 and (nbad == 4 or L >= 32)
    ph[0, 0], ph[n_ph // 2 if n_ph > 2 else 0, L - 1] = 0, V - 1
    for k, v in enumerate((-1, V, I32_MIN, I32_MAX)):
        ph[n_ph - 1 - k % nbad, (7 * k + 3) % L] = v
    return dict(logits=logits, lse=lse, idx=idx, codes=codes, inf_row=inf_row)


def _gathered(logits, codes, B, M, P, L, V, dtype, clamp=False, scenes=None):
    """z[b][m][p][t] = logits[row_t][c_t] as ``dtype`` and ok[b][1][p][t] = the code lies in [0, V); ``clamp``: the mistake"""
    ld = logits.shape[1]
    rows = logits.reshape(B, M, L, ld)
    z = np.empty((B, M, P, L), dtype=dtype)
    ok = np.empty((B, 1, P, L), dtype=bool)
    t = np.arange(L)[None, :]
    for b in range(B):
        cb = codes[(b if codes.shape[0] > 1 else 0) if scenes is None else scenes[b]].astype(np.int64)
        ok[b, 0] = (cb >= 0) & (cb < V) if not clamp else True
        z[b] = rows[b][:, t, np.clip(cb, 0, V - 1)].astype(dtype)
    return z, ok


def reference(inp, c):
    """float64 from the float32 inputs -> (log_likelihood [B][M][P], magnitude sum_t |z_t - lse_t|, accuracy), float64"""
    L, V, B, M, P = c['L'], c['V'], c['B'], c['M'], c['P']
    z, ok = _gathered(inp['logits'], inp['codes'], B, M, P, L, V, np.float64)
    lse = inp['lse'].astype(np.float64).reshape(B, M, 1, L)
    with np.errstate(invalid='ignore'):
        x = np.where(ok, z - lse, -np.inf)
        ll = x[..., 0].copy()
        for t in range(1, L):
            ll = ll + x[..., t]
        mag = np.abs(x).sum(-1)
    hits = (inp['idx'].reshape(B, M, 1, L) == inp['codes'].astype(np.int64)[_scene_index(inp['codes'], B)][:, None]).sum(-1)
    return ll, mag, hits / float(L)


def _scene_index(codes, B, scenes=None):
    return np.array([(b if codes.shape[0] > 1 else 0) if scenes is None else scenes[b] for b in range(B)])


def _pairwise32(x):
    """the float32 sum over the last axis as a balanced tree (what the chain is NOT)"""
    x = [x[..., t] for t in range(x.shape[-1])]
    while len(x) > 1:
        x = [(x[i] + x[i + 1]).astype(F32) if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
    return x[0]


def restated_f32(inp, c, mistake=None):
    """float32 in the kernel's order -> (log_likelihood, accuracy) fp32 [B][M][P]: x_t = fsub(z_t, lse_t) or -inf, s = x_0, s = fadd(s, x_t);
    accuracy = (float)hits / (float)L.  ``mistake``: one of MISTAKES, what the host test must see told apart."""
    assert mistake is None or mistake in MISTAKES
    L, V, B, M, P = c['L'], c['V'], c['B'], c['M'], c['P']
    codes = inp['codes']
    if mistake == 'next_photo':
        codes = np.roll(codes, -1, axis=1)
    scenes = [0] * B if mistake == 'ignore_stride' else None
    z, ok = _gathered(inp['logits'], codes, B, M, P, L, V, F32, clamp=mistake == 'clamp', scenes=scenes)
    lse = inp['lse'].reshape(B, M, 1, L)
    with np.errstate(invalid='ignore', over='ignore'):
        if mistake == 'sum_then_sub':
            zs, ls = np.where(ok, z, F32(-np.inf))[..., 0].copy(), np.broadcast_to(lse, z.shape)[..., 0].copy()
            for t in range(1, L):
                zs = (zs + np.where(ok, z, F32(-np.inf))[..., t]).astype(F32)
                ls = (ls + np.broadcast_to(lse, z.shape)[..., t]).astype(F32)
            ll = (zs - ls).astype(F32)
        else:
            x = np.where(ok, (z - lse).astype(F32), F32(-np.inf)).astype(F32)
            if mistake == 'pairwise':
                ll = _pairwise32(x)
            else:
                ll = x[..., 0].copy()
                for t in range(1, L):
                    ll = (ll + x[..., t]).astype(F32)
    hits = (inp['idx'].reshape(B, M, 1, L) == codes.astype(np.int64)[_scene_index(codes, B, scenes)][:, None]).sum(-1)
    acc = (hits.astype(F32) / F32(V if mistake == 'acc_over_V' else L)).astype(F32)
    if mistake == 'swap_pm':                                              # element (b, m, p) stored at [b][p][m] of the same buffer
        ll = np.ascontiguousarray(ll.transpose(0, 2, 1)).reshape(B, M, P)
        acc = np.ascontiguousarray(acc.transpose(0, 2, 1)).reshape(B, M, P)
    return np.ascontiguousarray(ll, dtype=F32), np.ascontiguousarray(acc, dtype=F32)


def applies(mistake, c):
    """the cases on which a mistake MUST show: where it computes something else than the kernel (another order of a sum shows in the last
    bit of some elements only: it is asked of the cases with long sums and thousands of elements)"""
    long_sums = c['L'] >= 64 and c['P'] >= 64
    return {'pairwise': long_sums, 'sum_then_sub': long_sums, 'swap_pm': c['M'] > 1 and c['P'] > 1, 'next_photo': c['P'] > 1,
            'clamp': True, 'ignore_stride': c['B'] > 1 and c['stride'] != 'shared', 'acc_over_V': c['V'] != c['L']}[mistake]


def bits(x):
    """int32 bit patterns of float32 ``x`` (a tensor or an array), every NaN mapped to 0x7FC00000 (see the module docstring)"""
    t = torch.as_tensor(np.ascontiguousarray(x) if not torch.is_tensor(x) else x).contiguous()
    assert t.dtype == torch.float32
    return torch.where(torch.isnan(t), torch.tensor(0x7FC00000, dtype=torch.int32, device=t.device), t.view(torch.int32))


def worst_ratio(got, want, mag, L):
    """max over the elements with a finite reference of |got - want| / (gamma_L x magnitude); the others must be matched as they are
    (-inf by -inf, NaN by NaN), else inf"""
    got, want, mag = (np.asarray(a, dtype=np.float64) for a in (got, want, mag))
    fin = np.isfinite(want)
    special_ok = np.array_equal(np.isnan(got[~fin]), np.isnan(want[~fin])) and np.array_equal(got[~fin][~np.isnan(want[~fin])],
                                                                                               want[~fin][~np.isnan(want[~fin])])
    if not special_ok or not np.isfinite(got[fin]).all():
        return float('inf')
    if not fin.any():
        return 0.0
    err, m = np.abs(got[fin] - want[fin]), mag[fin]
    r = np.where(m > 0, err / (gamma(L) * np.maximum(m, 1e-300)), np.where(err == 0, 0.0, np.inf))
    return float(r.max())
