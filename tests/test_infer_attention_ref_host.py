"""CPU: the references, restatements and cases of tests/infer_attention_ref.py.
1. the float64 references pinned against oracle/migt_oracle.py (compute_causal_block_attention and its multi-end form) on the 64-token
   cases, and the prefix reference (the twin-mask sequence) against the independent statement in the cache's own layout;
2. the input classes do what they are for (rising: the running maximum moves in every tile; falling: it sits in the first; deep: every
   visible score far below zero; peaked: one key leads by more than 20) and every case keeps the kernels' precondition (row maximum above
   -1e4 + 104, under which skip_masked = 1 and the dense form are the same bits);
3. the calibration the constants of tests/test_hip_infer_attention_kernels.py come from: per (kernel, case) the worst error of the
   restatement against float64 in the arm's unit x magnitude, c = 4 x the worst basis rounded up to a power of two, the bases of an arm
   within one decade across the input classes;
4. the comparison with that c rejects the ways these kernels go wrong.

On the decade.  The score term of P's magnitude states what rounding q and k to the arm's format costs.  With bf16-exact operands that
rounding never happens in the lp and prefix-bf16 kernels (they round the UN-scaled q; the training kernel rounds q scale log2 e), and their
bases then fall as 1 / (1 + 2 s_abs): 0.44 at scale 0.125 against 0.02 at |s| ~ 40.  The magnitude misses no term there; the inputs miss
the rounding.  Both kernels therefore also run a form with fp32 operands that are NOT bf16 numbers, which is what the fp32 transformer arm
hands them, and the basis of a case is the worst over its forms.  The 'peaked' class is outside the decade from BELOW in every arm and is
asserted separately to stay below the arm's worst: with a lead of more than 20 every other weight is below e^-20 < 2^-24, out is the
leader's v, and no rounding of the softmax is left to measure."""
import functools

import numpy as np
import pytest
import torch

import attention_kernels_ref as A
import infer_attention_ref as I
import test_attention_kernels_ref_host as TH

F64 = torch.float64
ARMS = ('x6', 'lp', 'fp8')


def _pow2_ceil(x):
    return 2.0 ** int(np.ceil(np.log2(x)))


# ------------------------------------------------------------------ 1. references
@pytest.mark.parametrize('name', [c[0] for c in I.BC_CASES if c[4] == 64 and c[3] % 64 == 0])
def test_blockcausal_reference_against_the_oracle(name):
    case = I.BC_BY_NAME[name]
    _, B, H, T, L, spec, scale, kind = case
    q, k, v = I.bc_inputs(case, 'x6')
    _, (val, mag) = I.bc_reference(case, 'x6')
    qh, kh, vh = (A.heads(x, B, H, T) for x in (q, k, v))
    want = TH._oracle_attention(qh * float(np.float32(scale)), kh, vh, B, H, T // L, L, spec, None)
    assert TH._within(val, A.rows(want), mag), name


@functools.lru_cache(maxsize=None)
def _pref(name, exact16):
    return I.prefix_reference(I.PREFIX_BY_NAME[name], exact16)


def _flat_cache(x, B, C, d, ldkp, ldvp, pstride):
    """kp / vp as FLAT buffers in the layout the entry points take, NaN between the logical elements"""
    n = (B - 1) * pstride + C * I.LV * max(ldkp, ldvp)
    kp, vp = torch.full((n,), float('nan')), torch.full((n,), float('nan'))
    for b in range(B):
        for r in range(C * I.LV):
            kp[b * pstride + r * ldkp:b * pstride + r * ldkp + d] = x['kp'][b, r]
            vp[b * pstride + r * ldvp:b * pstride + r * ldvp + d] = x['vp'][b, r]
    return kp, vp


@pytest.mark.parametrize('name', [c[0] for c in I.PREFIX_CASES if c[2] <= 5])
def test_prefix_reference_against_the_independent_statement_and_the_oracle(name):
    from oracle import migt_oracle as mg
    case = I.PREFIX_BY_NAME[name]
    _, B, C, N, kind, layout, lens = case
    H, d = I.PREFIX_H, I.PREFIX_H * I.DH
    x = I.prefix_inputs(case, False)
    val, mag = _pref(name, False)
    assert not torch.isnan(val).any()
    for ldkp, ldvp, pstride in ((d, d, C * I.LV * d), (d + 8, d + 24, C * I.LV * (d + 24) + 40)):
        kp, vp = _flat_cache(x, B, C, d, ldkp, ldvp, pstride)
        got = I.prefix_fp64(x['q'], x['k'], x['v'], kp, vp, B, H, C, N, ldkp, ldvp, pstride, lens)
        assert TH._within(got, val, mag), (name, ldkp, ldvp, pstride)
    # the oracle: an ending sees the views of its context and itself (compute_causal_block_attention with one query view)
    for b in range(B):
        for n in range(N):
            c = C if lens is None else lens[b][n]
            sl = slice((b * N + n) * I.LV, (b * N + n + 1) * I.LV)

            def views(pre, own):
                t = torch.cat([pre[b, :c * I.LV], own[sl]]).to(F64)
                return t.reshape(1, c + 1, I.LV, H, I.DH).permute(0, 3, 1, 2, 4)
            qv = x['q'][sl].to(F64).reshape(1, 1, I.LV, H, I.DH).permute(0, 3, 1, 2, 4)
            o = mg.compute_causal_block_attention(views(x['kp'], x['k']), views(x['vp'], x['v']), qv)       # [1][H][1][L][64]
            assert TH._within(val[sl], o[0, :, 0].permute(1, 0, 2).reshape(I.LV, d), mag[sl]), (name, b, n)


# ------------------------------------------------------------------ 2. the classes and the precondition
@functools.lru_cache(maxsize=None)
def _bref(arm, name):
    return I.bc_reference(I.BC_BY_NAME[name], arm)


@pytest.mark.parametrize('name', [c[0] for c in I.BC_CASES])
def test_precondition_of_skip_equals_dense(name):
    """a masked weight is an exact zero whenever the row maximum exceeds -1e4 + 104: every case and arm, 'deep' included"""
    for arm in ARMS:
        ref, _ = _bref(arm, name)
        assert float(ref.row_max.min()) > -1e4 + 104, (arm, name, float(ref.row_max.min()))


@pytest.mark.parametrize('name', [c[0] for c in I.BC_CASES if c[7] in ('rising', 'falling', 'deep', 'peaked')])
def test_input_classes_do_what_they_are_for(name):
    case = I.BC_BY_NAME[name]
    _, B, H, T, L, spec, scale, kind = case
    for arm in ('x6', 'lp'):
        q, k, v = I.bc_inputs(case, arm)
        tm = I.tile_maxima(q, k, B, H, T, L, spec, scale)                       # [B][H][T][ntiles], -inf = no visible key
        seen = torch.isfinite(tm)
        run = torch.cummax(tm, -1).values
        moved = seen[..., 1:] & (tm[..., 1:] > run[..., :-1])
        later = seen[..., 1:] & torch.isfinite(run[..., :-1])                   # tiles that follow a tile with a visible key
        if kind == 'rising':
            frac = float(moved.sum()) / float(later.sum())
            print(f'{name} [{arm}]: the running maximum moves in {frac:.4f} of the later visible tiles')
            assert frac > 0.97
        elif kind == 'falling':
            frac = float((moved & later).sum()) / float(later.sum())
            print(f'{name} [{arm}]: the running maximum moves in {frac:.4f} of the later visible tiles')
            assert frac < 0.03
        elif kind == 'deep':
            top = float(tm[seen].max())
            print(f'{name} [{arm}]: the largest visible score is {top:.1f}')
            assert top < -25.0
        else:
            qh, kh = A.heads(q, B, H, T), A.heads(k, B, H, T)
            s = qh @ kh.transpose(-1, -2) * float(np.float32(scale))
            vis = A.token_mask(T, L, spec)
            s = torch.where(vis, s, torch.full_like(s, float('-inf')))
            top2 = torch.topk(s, 2, -1).values
            lead = float((top2[..., 0] - top2[..., 1]).min())
            print(f'{name} [{arm}]: the smallest lead of a row is {lead:.1f}')
            assert lead > 20.0 and bool((s.argmax(-1) == torch.arange(T)).all())


# ------------------------------------------------------------------ 3. calibration
def _calibrate_bc(case):
    name, B, H, T, L, spec, scale, kind = case
    res = {}
    q, k, v = I.bc_inputs(case, 'x6')
    _, (val, mag) = _bref('x6', name)
    res['x6'] = A.ratio(I.fwd_x6(q, k, v, B, H, T, L, spec, scale), val, mag, I.U32)
    # lp: the exact-operand forms (bf16 in and fp32 in of the same values are one restatement) and the raw fp32 operands, each with both outs
    worst = 0.0
    for arm_in, (rv, rm) in (('lp', _bref('lp', name)[1]), ('x6', (val, mag))):
        ql, kl, vl = I.bc_inputs(case, arm_in)
        for ob in (False, True):
            worst = max(worst, A.ratio(I.fwd_lp(ql, kl, vl, B, H, T, L, spec, scale, out_bf16=ob), rv, rm, I.U16))
    res['lp'] = worst
    q8, k8, v8 = I.bc_inputs(case, 'fp8')
    _, (val8, mag8) = _bref('fp8', name)
    res['fp8'] = max(A.ratio(I.fwd_lp(q8, k8, v8, B, H, T, L, spec, scale, out_bf16=ob, fp8=True), val8, mag8, I.U8) for ob in (False, True))
    return res


def _calibrate_prefix(case):
    name, B, C, N, kind, layout, lens = case
    res = {}
    worst = 0.0
    for exact in (True, False):
        x = I.prefix_inputs(case, exact)
        val, mag = _pref(name, exact)
        for ob in (False, True):
            worst = max(worst, A.ratio(I.prefix_restate('prefix bf16', x, B, C, N, lens, ob), val, mag, I.U16))
        if not exact:
            res['prefix f32eq'] = A.ratio(I.prefix_restate('prefix f32eq', x, B, C, N, lens), val, mag, I.U32)
    res['prefix bf16'] = worst
    return res


_CAL = {}


def _cal(name):
    if name not in _CAL:
        _CAL[name] = _calibrate_bc(I.BC_BY_NAME[name]) if name in I.BC_BY_NAME else _calibrate_prefix(I.PREFIX_BY_NAME[name])
    return _CAL[name]


@pytest.mark.parametrize('name', [c[0] for c in I.BC_CASES] + [c[0] for c in I.PREFIX_CASES])
def test_calibration_per_case(name):
    res = _cal(name)
    print(f'basis [{name}]: ' + '  '.join(f'{k} {v:.3g}' for k, v in res.items()))
    assert all(np.isfinite(v) for v in res.values())


def _kind(name):
    return (I.BC_BY_NAME[name][7] if name in I.BC_BY_NAME else I.PREFIX_BY_NAME[name][4])


def test_calibration_covers_the_gpu_tests_constants():
    """c = 4 x the restatement's worst error over the cases, rounded up to a power of two; the basis beside it in the GPU test's table is
    this run's (a float32 sum depends on how torch splits it: the table may sit one binade from this run's figure, never further).  Per
    arm the bases stay within one decade over the cases of every class but 'peaked', which must stay below the arm's worst (module
    docstring)."""
    import test_hip_infer_attention_kernels as G
    names = [c[0] for c in I.BC_CASES] + [c[0] for c in I.PREFIX_CASES]
    per_arm = {}
    for n in names:
        for arm, v in _cal(n).items():
            per_arm.setdefault(arm, []).append((n, v))
    assert set(per_arm) == set(G.C)
    for arm in sorted(per_arm):
        worst = max(v for n, v in per_arm[arm])
        print(f'calibration {arm}: restatement worst {worst:.3g} units -> c = {_pow2_ceil(4 * worst):g} (table: c = {G.C[arm]:g}, basis {G.BASIS[arm]:g})')
        assert G.C[arm] == _pow2_ceil(4 * G.BASIS[arm]), arm
        assert _pow2_ceil(4 * worst) <= 2 * G.C[arm] and G.C[arm] <= 2 * _pow2_ceil(4 * worst), (arm, worst, G.C[arm])
        rounded = [v for n, v in per_arm[arm] if _kind(n) != 'peaked']
        peaked = [v for n, v in per_arm[arm] if _kind(n) == 'peaked']
        lo_n, lo = min(((n, v) for n, v in per_arm[arm] if _kind(n) != 'peaked'), key=lambda t: t[1])
        print(f'{arm}: basis per case from {min(rounded):.3g} ({lo_n}) to {max(rounded):.3g}; peaked {min(peaked):.3g} .. {max(peaked):.3g}')
        assert max(rounded) <= 10 * min(rounded), (arm, min(rounded), max(rounded))
        assert max(peaked) <= max(rounded), (arm, peaked)


# ------------------------------------------------------------------ 4. mutants
# Every mutant is rejected by x6 / f32eq on each of its cases and by the bf16 arms on the case named for it.  What the low-precision arms
# cannot reject is printed with "not asserted", and the reason is always the same one: their unit times the magnitude's score term
# (1 + 2 s_abs) is the error the arm's own operand rounding is entitled to, and a mutant that moves a row's weights by less than that is
# inside it.  For fp8 (unit 2^-4, c = 2) that allowance reaches the whole of sum P |v| once s_abs > 3.5: it rejects the mutants that wreck
# a row (streams, the skipped rescale, the missing clamp) and no mutant that adds or drops a few keys of a diffuse row.
def _C(arm):
    import test_hip_infer_attention_kernels as G
    return G.C[arm]


def _rejected(arm, got, val, mag, what, asserted=True):
    r = A.ratio(got, val, mag, I.UNIT[arm])
    print(f'mutant [{what}] {arm}: {r:.3g} units (c = {_C(arm):g})' + ('' if asserted else ', not asserted'))
    if asserted:
        assert not r <= _C(arm), (what, arm, r, _C(arm))


def _bc_mutant_vis(name, vm, what, asserted):
    case = I.BC_BY_NAME[name]
    _, B, H, T, L, spec, scale, kind = case
    for arm in ARMS:
        _, (val, mag) = _bref(arm, name)
        _, (mval, _) = I.bc_reference(case, arm, mut={'vis': A.token_mask(T, L, spec, views=vm)})
        _rejected(arm, mval, val, mag, f'{what}: {name}', arm in asserted)


@pytest.mark.parametrize('name', ['B2 C2 N3', 'B1 C3 N4 deep', 'B1 C19 N2', 'B2 C2 N3 peaked'])
def test_mutant_one_prefix_key_dropped_for_one_view(name):
    """the last query view never sees the last key of the last prefix view (the probe of the issue)"""
    case = I.PREFIX_BY_NAME[name]
    _, B, C, N, kind, layout, lens = case
    H, T = I.PREFIX_H, (C + N) * I.LV
    vis = I.prefix_vis(C, N, [C] * N).clone()
    vis[(C + N - 1) * I.LV:, C * I.LV - 1] = False
    for arm, exact in (('prefix bf16', True), ('prefix f32eq', False)):
        x = I.prefix_inputs(case, exact)
        val, mag = _pref(name, exact)
        qs, ks, vs = I.prefix_sequence(x, B, C, N)
        mval = torch.cat([A.Ref(qs[b * T:(b + 1) * T], ks[b * T:(b + 1) * T], vs[b * T:(b + 1) * T], None, 1, H, T, I.LV, C, 1.0,
                                mut={'vis': vis}).out[0][C * I.LV:] for b in range(B)])
        # peaked: the dropped key's weight is below e^-20, out does not hold it in either arm; deep: one of 256 near-equal weights, 0.4 % of
        # a row, against the 18 % that 2^-9 (1 + 2 s_abs) allows the bf16 arm at s_abs ~ 45
        _rejected(arm, mval, val, mag, f'one prefix key dropped: {name}', kind == 'init' or (kind == 'deep' and arm == 'prefix f32eq'))


@pytest.mark.parametrize('name', ['T256 L64 twin0', 'T70 L7 twin8', 'T320 L64 twin3 rising'])
def test_mutant_a_sibling_twin_visible(name):
    _, B, H, T, L, spec, scale, kind = I.BC_BY_NAME[name]
    nv = (T + L - 1) // L
    vm = A.view_matrix(nv, spec).clone()
    assert not bool(vm[nv - 1, spec])
    vm[nv - 1, spec] = True                                                      # the last ending sees the first one
    _bc_mutant_vis(name, vm, 'a sibling twin visible', {'T256 L64 twin0': ARMS, 'T70 L7 twin8': ('x6', 'lp')}.get(name, ('x6',)))


@pytest.mark.parametrize('name', ['T256 L64 streams2x2 s1.7', 'T240 L16 streams3x5 s.125', 'T640 L64 streams5x2 s.125'])
def test_mutant_branch_view_sees_its_own_index_in_the_main_stream(name):
    _, B, H, T, L, spec, scale, kind = I.BC_BY_NAME[name]
    Sv, nv = -spec, T // L
    qv, kv = torch.arange(nv)[:, None], torch.arange(nv)[None, :]
    vm = torch.where(qv // Sv == 0, (kv // Sv == 0) & (kv % Sv <= qv % Sv), ((kv // Sv == 0) & (kv % Sv <= qv % Sv)) | (kv == qv))
    assert int((vm != A.view_matrix(nv, spec)).sum()) == (nv // Sv - 1) * Sv
    _bc_mutant_vis(name, vm, 'ki <= qi for streams >= 1', ARMS)


@pytest.mark.parametrize('name', ['T100 none deep', 'T70 none s1.7', 'T129 none s.125'])
def test_mutant_phantom_zero_score_key_at_index_T(name):
    """a zero-filled key row at index T taken as a key: score 0, v = 0.  In the 'deep' class it takes the whole row (every real score is
    below -30) and the bf16 arm rejects it; among scores of a few units it is one key in T"""
    case = I.BC_BY_NAME[name]
    _, B, H, T, L, spec, scale, kind = case
    assert L == 0
    for arm in ARMS:
        q, k, v = I.bc_inputs(case, arm)
        _, (val, mag) = _bref(arm, name)

        def ext(x):
            return torch.cat([x.reshape(B, T, -1), torch.zeros((B, 1, x.shape[1]))], 1).reshape(B * (T + 1), -1)
        mval = A.Ref(ext(q), ext(k), ext(v), None, B, H, T + 1, 0, -1, scale).out[0].reshape(B, T + 1, -1)[:, :T].reshape(B * T, -1)
        _rejected(arm, mval, val, mag, f'phantom key at T: {name}', arm == 'x6' or (arm == 'lp' and kind == 'deep'))


@pytest.mark.parametrize('name', ['T320 L64 twin3 rising', 'T240 L48 causal rising'])
def test_mutant_rescale_skipped(name):
    case = I.BC_BY_NAME[name]
    _, B, H, T, L, spec, scale, kind = case
    for arm in ARMS:
        q, k, v = I.bc_inputs(case, arm)
        _, (val, mag) = _bref(arm, name)
        _rejected(arm, I.out_rescale_skipped(q, k, v, B, H, T, L, spec, scale), val, mag, f'rescale skipped: {name}')
    # in the falling class the same mutant is harmless: that is why the rising class exists
    fname = name.replace('rising', 'falling')
    fcase = I.BC_BY_NAME[fname]
    q, k, v = I.bc_inputs(fcase, 'lp')
    _, (val, mag) = _bref('lp', fname)
    r = A.ratio(I.out_rescale_skipped(q, k, v, *fcase[1:7]), val, mag, I.U16)
    print(f'mutant [rescale skipped: {fname}] lp: {r:.3g} units')


def test_mutant_masked_scores_at_minus_1e4_times_scale():
    """the lp kernel writes the masked score in units of the raw score, -1e4 / scale; -1e4 (that is -1e4 x scale after scaling) leaks at
    scale 2^-14.  At the suite's other scales (0.125 .. 1.7) the mutant's weights still underflow and it is the same function: the case
    'T144 L48 causal s2^-14' was added for this mutant."""
    name = 'T144 L48 causal s2^-14'
    case = I.BC_BY_NAME[name]
    _, B, H, T, L, spec, scale, kind = case
    vis = A.token_mask(T, L, spec).to(F64)
    for arm in ARMS:
        q, k, v = I.bc_inputs(case, arm)
        if arm == 'fp8':
            q, k, v = I.clamp8(q), I.clamp8(k), I.clamp8(v)
        _, (val, mag) = _bref(arm, name)
        qh, kh, vh = (A.heads(x, B, H, T) for x in (q, k, v))
        s = scale * (qh @ kh.transpose(-1, -2))
        s = s * vis - 1e4 * scale * (1 - vis)
        _rejected(arm, A.rows(torch.softmax(s, -1) @ vh), val, mag, 'masked at -1e4 x scale')
    other = I.BC_BY_NAME['T240 L16 streams3x5 s.125']
    assert float(np.exp(-1e4 * other[6] + 200.0)) == 0.0


@pytest.mark.parametrize('name', ['B2 C5 N2 var', 'B1 C3 N4 var'])
def test_mutant_var_view_reads_one_view_past_its_length(name):
    case = I.PREFIX_BY_NAME[name]
    _, B, C, N, kind, layout, lens = case
    for b in range(B):
        for n in range(N):
            if lens[b][n] >= C:
                continue
            bad = [list(row) for row in lens]
            bad[b][n] += 1
            for arm, exact in (('prefix bf16', True), ('prefix f32eq', False)):
                val, mag = _pref(name, exact)
                mval, _ = I.prefix_reference(case, exact, lens=bad)
                _rejected(arm, mval, val, mag, f'{name}: view ({b}, {n}) reads {bad[b][n]} views instead of {lens[b][n]}')


def test_mutant_fp8_without_the_clamp():
    """v_cvt_pk_fp8_f32 does not saturate.  No operand of the 'large' class is anywhere near 448, so on it the mutant is the same function:
    the fp8 arm runs 'T256 L64 causal large' with four operands beyond +-448 (class 'largeclamp'), the case changed for this mutant."""
    case = I.BC_BY_NAME[I.FP8_LARGE]
    _, B, H, T, L, spec, scale, kind = case
    q, k, v = I.bc_inputs(case, 'fp8')
    assert float(v.abs().max()) > I.E4M3_MAX and float(q.abs().max()) > I.E4M3_MAX
    ql, kl, vl = I.bc_inputs(case, 'lp')
    assert float(torch.stack([ql.abs().max(), kl.abs().max(), vl.abs().max()]).max()) < 8.0
    _, (val, mag) = _bref('fp8', I.FP8_LARGE)
    _rejected('fp8', I.fwd_lp(q, k, v, B, H, T, L, spec, scale, fp8=True, clamp=False), val, mag, 'fp8 without the clamp')


def test_fp8_floor_term():
    """FLOOR8 from the format: e4m3fn's smallest normal number and subnormal step as torch holds them, at the carried scale 2^8"""
    fi = torch.finfo(torch.float8_e4m3fn)
    assert fi.smallest_normal == 2.0 ** -6 and fi.eps == 2.0 ** -3 and fi.max == I.E4M3_MAX
    step = fi.smallest_normal * fi.eps                                          # subnormals are multiples of 2^-9
    assert I.FLOOR8 == (step / 2 / I.P_SCALE_FP8) / I.U8 == 2.0 ** -14
    assert I.U8 == fi.eps / 2
    x = torch.tensor([2.0 ** -10 * 1.01, 2.0 ** -10 * 0.99, 3 * 2.0 ** -9 + 2.0 ** -11])
    assert I.e4m3(x).tolist() == [2.0 ** -9, 0.0, 3 * 2.0 ** -9]
    assert torch.isnan(I.e4m3(torch.tensor([1000.0, -470.0]))).all() and I.e4m3(torch.tensor([460.0])).item() == 448.0
