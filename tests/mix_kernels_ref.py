"""References for the mean-view kernel (csrc/mix_rows.hip): the float64 reference of include/vf_hip.h's contract — the sampler's kept set
(``sample_kernels_ref.sample_ref``), p = the soft-max over it, out = E p — with a magnitude per output element; the float32 restatement
of the kernel in its own order of operations; the usual mistakes as float64 mutants; the inputs and the case table of
tests/test_hip_mix_rows.py.  tests/test_mix_ref_host.py pins all of it on the CPU.

Magnitude of out[d] (what 2^-24 is multiplied with): the reference expression with every summand's absolute value, each exponential judged
against p_n (1 + |z_n - max z| / T) as tests/score_kernels_ref.py judges them (an exponential's relative error grows with its argument's
rounding), and the same term once more for the normalising sum, which every summand is divided by:
    mag[d] = sum_n p_n (1 + |y_n - m|) |E[d][n]|  +  (sum_n p_n |E[d][n]|) (sum_n p_n (1 + |y_n - m|))
The constant c in front is calibrated on the float32 restatement (``C_OUT`` below), never on the kernel."""
import math

import numpy as np
import torch

import sample_kernels_ref as R
from training_kernels_ref import U, rng  # noqa: F401

F32, F64 = np.float32, np.float64
ROWS_PER_GROUP = 16                       # R: the rows that share one workgroup (ops.MIX_ROWS_PER_GROUP)
PAD_E = 3                                 # columns of NaN behind E's N codes in the padded layout
# (basis, c): the worst deviation of mix_f32 from mix_ref over the GPU test's own inputs in units of 2^-24 x magnitude, as
# tests/test_mix_ref_host.py measures it, and c = 4 x basis rounded up to a power of two (DESIGN.md §6.14's rule)
C_OUT = (3.77, 16.0)


def kept_set(z, temperature=1.0, top_k=0, top_p=1.0):
    """the sampler's kept set of every row: bool [rows][N]"""
    return R.sample_ref(np.asarray(z, dtype=F32), temperature, top_k, top_p, 0, None, 1)['keep']


def keep_from_count(z, kept):
    """the kept set from its size: a kept set is a threshold on the row's values (ties kept), so its size names it"""
    z = np.asarray(z, dtype=F32).astype(F64)
    srt = -np.sort(-z, 1)
    kept = np.asarray(kept).astype(np.int64)
    thr = np.take_along_axis(srt, np.clip(kept - 1, 0, z.shape[1] - 1)[:, None], 1)
    return (z >= thr) & (z > -math.inf) & (kept > 0)[:, None]


def mix_ref(z, E, temperature=1.0, top_k=0, top_p=1.0, keep=None):
    """z [rows][N] float32, E [D][N] float32 -> dict(out float64 [rows][D] (NaN rows: no finite logit), mag float64 [rows][D], p float64
    [rows][N], keep, kept int32 [rows]); ``keep``: a kept set to use instead of the reference's own"""
    z = np.asarray(z, dtype=F32).astype(F64)
    E = np.asarray(E, dtype=F32).astype(F64)
    T = float(F32(temperature))
    keep = kept_set(z, temperature, top_k, top_p) if keep is None else np.asarray(keep, dtype=bool)
    empty = ~keep.any(1)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        y = z / T
        m = np.where(empty, 0.0, np.where(np.isfinite(y), y, -math.inf).max(1))      # the row's maximum: always kept
        d = np.where(keep, y - m[:, None], 0.0)
        e = np.where(keep, np.exp(d), 0.0)
        s = e.sum(1)
        p = e / np.where(empty, 1.0, s)[:, None]
        out = p @ E.T
        w = p * (1.0 + np.abs(d))
        mag = w @ np.abs(E).T + (p @ np.abs(E).T) * w.sum(1)[:, None]
    out[empty] = math.nan
    return dict(out=out, mag=mag, p=p, keep=keep, kept=keep.sum(1).astype(np.int32), empty=empty)


def mix_f32(z, E, temperature=1.0, top_k=0, top_p=1.0):
    """the kernel in float32, in its order: the sampler's restatement for the kept set, e and the mass (``sample_f32``: d = (z - max z) / T,
    e = e^d once per row, the mass in lane order then the butterfly); p = fl(e / mass) on the kept set, +0 elsewhere; out[d] = ONE chain
    acc = fma(p_n, E[d][n], acc) from +0 over n ascending (the product is exact in float64; the sum is rounded to float32 once more than
    an fma would, which moves a last bit in rare cases — this restatement calibrates a tolerance, it is not compared bit for bit)"""
    z = np.asarray(z, dtype=F32)
    E32 = np.asarray(E, dtype=F32)
    r = R.sample_f32(z, temperature, top_k, top_p, 0, None, 1)
    keep, e = r['keep'], r['e']
    with np.errstate(invalid='ignore', divide='ignore', under='ignore'):
        mass = R._mass32(e, keep)
        p = np.where(keep, (e / np.where(mass > 0, mass, F32(1))[:, None]).astype(F32), F32(0)).astype(F32)
        acc = np.zeros((z.shape[0], E32.shape[0]), F32)
        E64 = E32.astype(F64)
        for n in range(z.shape[1]):
            if p[:, n].any():
                acc = (p[:, n].astype(F64)[:, None] * E64[None, :, n] + acc.astype(F64)).astype(F32)
    empty = ~keep.any(1)
    acc[empty] = np.nan
    return dict(out=acc, p=p, keep=keep, kept=np.where(empty, 0, keep.sum(1)).astype(np.int32), thr=r['thr'])


MISTAKES = ('temperature_last', 'unfiltered_sum', 'p_before_k', 'strict', 'tile_dropped', 'E_transposed')


def mix_mutant(z, E, temperature, top_k, top_p, mistake):
    """float64 [rows][D]: the reference with one mistake (what the host test must see rejected)"""
    assert mistake in MISTAKES
    z64 = np.asarray(z, dtype=F32).astype(F64)
    E64 = np.asarray(E, dtype=F32).astype(F64)
    D, N = E64.shape
    T = float(F32(temperature))
    keep = kept_set(z, temperature, top_k, top_p)
    if mistake == 'temperature_last':                                               # the filters see z, the soft-max z / T
        keep = kept_set(z, 1.0, top_k, top_p)
    elif mistake == 'p_before_k':                                                   # the nucleus of the whole row, then top-k
        keep = kept_set(z, temperature, 0, top_p) & kept_set(z, temperature, top_k, 1.0)
    elif mistake == 'strict':                                                       # ties at the threshold dropped (the maximum stays)
        y = np.where(keep, z64, math.inf)
        keep = keep & ((z64 > y.min(1, keepdims=True)) | (z64 == z64.max(1, keepdims=True)))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        y = z64 / T
        m = np.where(np.isfinite(y), y, -math.inf).max(1)
        e = np.where(keep, np.exp(y - m[:, None]), 0.0)
        s = np.where(np.isfinite(y), np.exp(y - m[:, None]), 0.0).sum(1) if mistake == 'unfiltered_sum' else e.sum(1)
        p = e / s[:, None]
    if mistake == 'tile_dropped':                                                   # the 32 codes around each row's most likely one
        t0 = p.argmax(1) // 32 * 32
        p = np.where((np.arange(N)[None] >= t0[:, None]) & (np.arange(N)[None] < t0[:, None] + 32), 0.0, p)
    if mistake == 'E_transposed':                                                   # E read as [N][D]
        E64 = E64.reshape(-1)[:N * D].reshape(N, D).T
    return p @ E64.T


def worst_ratio(got, ref):
    """max over the elements of |got - ref.out| / (2^-24 x ref.mag); inf where a NaN is not met by a NaN or a value is not finite"""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got).astype(F64)
    out, mag = ref['out'], ref['mag']
    nan = np.isnan(out)
    if not np.array_equal(np.isnan(got), nan):
        return math.inf
    if nan.all():
        return 0.0
    err = np.abs(got - out)[~nan]
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err == 0, 0.0, err / (U * mag[~nan]))
    return float(ratio.max())


# ------------------------------------------------------------------ inputs and cases
NS = (1, 63, 64, 65, 128, 1024)
DS = (32, 256)
ROWS = (1, 3, ROWS_PER_GROUP - 1, ROWS_PER_GROUP, ROWS_PER_GROUP + 1, 2 * ROWS_PER_GROUP + 1)
TS = R.TS
TOP_PS = R.TOP_PS
top_ks = R.top_ks


def codebook(D, N, seed=0, integer=False):
    """E float32 [D][N + PAD_E]: N(0, 1) (or integers in [-8, 8]) with NaN in the pad columns — a read past N poisons the output"""
    g = rng(7000 + 13 * D + N + seed)
    E = np.full((D, N + PAD_E), np.nan, F32)
    E[:, :N] = g.integers(-8, 9, size=(D, N)).astype(F32) if integer else g.standard_normal((D, N)).astype(F32)
    return torch.from_numpy(E)


def cases(N):
    """every (top_k, top_p) pair of the lists at this N; rows, D, T, the layout and the kinds' shift walk their lists with the case number,
    so that every value of every dimension meets every N: (rows, N, D, T, top_k, top_p, padded, shift)"""
    out = []
    i = NS.index(N)
    for ki, top_k in enumerate(top_ks(N)):
        for pi, top_p in enumerate(TOP_PS):
            out.append((ROWS[i % 6], N, DS[(i // 2) % 2], TS[(i // 3) % 3], top_k, top_p, bool((ki + pi) % 2), i % len(R.KINDS)))
            i += 1
    return out


def all_cases():
    return [c for N in NS for c in cases(N)]


def inputs_for(case):
    """(x [rows][N + R.PAD] with +3e38 in the pad, E [D][N + PAD_E] with NaN in the pad, kinds)"""
    rows, N, D, T, top_k, top_p, padded, shift = case
    x, kinds, _ = R.inputs(rows, N, shift)
    return x, codebook(D, N), kinds


def reference_for(case, keep=None):
    rows, N, D, T, top_k, top_p, padded, shift = case
    x, E, kinds = inputs_for(case)
    return x, E, kinds, mix_ref(x[:, :N].numpy(), E[:, :N].numpy(), T, top_k, top_p, keep=keep)


def exact_cases():
    """the exact class: all-equal rows that keep all N codes (no filter, a top-p whose ties are kept, a top-k at a tie) and integer E in
    [-8, 8] — p = 1 / N, every product and partial sum is an integer / N below 2^24: out equals the float64 value exactly
    -> (rows, N, D, T, top_k, top_p)"""
    return [(rows, N, D, T, top_k, top_p) for N in (64, 1024) for rows, D, T, top_k, top_p in
            ((1, 32, 1.0, 0, 1.0), (ROWS_PER_GROUP + 1, 256, 0.5, 0, 0.5), (3, 32, 2.0, 2, 0.9))]


def exact_inputs(case):
    rows, N, D, T, top_k, top_p = case
    z = np.full((rows, N), 1.5, F32)
    E = codebook(D, N, seed=5, integer=True)
    ref = mix_ref(z, E[:, :N].numpy(), T, top_k, top_p)
    assert (ref['kept'] == N).all()
    return torch.from_numpy(z), E, ref
