"""CPU: the float64 references of tests/attention_kernels_ref.py pinned against independent statements (fp64 autograd of a dense masked
softmax attention; oracle/migt_oracle.py's compute_causal_block_attention / compute_causal_block_multiend_attention with and without
oracle/train_oracle.DropoutMasks; the oracle's masks for every (nviews <= 12, spec)), the kernels' precondition asserted on the reference
for every case, the calibration that the constants of tests/test_hip_attention_kernels.py come from (the CPU restatement of every entry
point against float64 on the GPU test's own inputs, in units of 2^-24 resp. 2^-9 x magnitude), the comparison checked against the ways
these kernels go wrong, and the host-side launch schedulers of csrc/vf_common.h walked by a sanitized stand-alone program."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import attention_kernels_ref as A
import training_kernels_ref as R

F64 = torch.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pow2_ceil(x):
    return 2.0 ** int(np.ceil(np.log2(x)))


def _within(got, want, mag, tol=1e-12):
    got, want, mag = R.t64(got), R.t64(want), R.t64(mag)
    return got.shape == want.shape and bool(((got - want).abs() <= tol * mag).all())


# ------------------------------------------------------------------ 1. the visibility restatement
def _oracle_views(nv, spec):
    """the oracle's mask as it acts: one token per view, q = k = 0 (uniform weights over the visible keys), v = one-hot of the key view"""
    from oracle import migt_oracle as mg
    eye = torch.eye(nv, dtype=F64)

    def z(n):
        return torch.zeros((1, 1, n, 1, nv), dtype=F64)

    def vv(idx):
        return eye[idx].reshape(1, 1, len(idx), 1, nv)
    if spec <= -2:
        Sv, NS = -spec, nv // -spec
        outs = mg.compute_causal_block_multiend_attention([z(Sv)] * NS, [vv(list(range(s * Sv, (s + 1) * Sv))) for s in range(NS)], [z(Sv)] * NS)
        return torch.cat([o.reshape(Sv, nv) for o in outs]) > 0
    Vc = nv if spec < 0 else min(spec, nv)
    parts = []
    if Vc:
        parts.append(mg.compute_causal_block_attention(z(Vc), vv(list(range(Vc))), z(Vc)).reshape(Vc, nv))
    for e in range(Vc, nv):                                                      # an ending: the common prefix and itself
        parts.append(mg.compute_causal_block_attention(z(Vc + 1), vv(list(range(Vc)) + [e]), z(1)).reshape(1, nv))
    return torch.cat(parts) > 0


def _specs(nv):
    return [-1] + list(range(0, nv + 2)) + [-Sv for Sv in range(2, nv + 1) if nv % Sv == 0]


def test_visibility_against_the_oracles_masks():
    n = 0
    for nv in range(1, 13):
        for spec in _specs(nv):
            vm = A.view_matrix(nv, spec)
            scalar = torch.tensor([[A.visible(q, k, spec) for k in range(nv)] for q in range(nv)])
            assert torch.equal(vm, scalar), (nv, spec)
            assert torch.equal(vm, _oracle_views(nv, spec)), (nv, spec)
            n += 1
    assert n > 130
    # streams with a view count that is no multiple of Sv, and wide twins: the scalar form is the definition
    for nv, spec in [(7, -3), (64, -16), (64, -32), (64, 62), (64, -1), (5, 9)]:
        vm = A.view_matrix(nv, spec)
        assert all(bool(vm[q, k]) == A.visible(q, k, spec) for q in range(nv) for k in range(nv))
    assert A.token_mask(70, 0, -1) is None
    tm = A.token_mask(70, 7, 8)
    assert tm.shape == (70, 70) and bool(tm[69, 0]) and not bool(tm[0, 69]) and bool(tm[63, 56]) == A.visible(9, 8, 8)


def test_dropout_mask_restatement_against_hash_py():
    """keep_mask writes the group index out (plane << 32 | q ceil(T/4) + (k >> 2), position k & 3): the same groups as _hash.attn_group, the
    same masks as train_oracle.dropout_keep, and drop_plane0 shifts the plane"""
    from viewformer_amd import _hash as hh
    from oracle.train_oracle import dropout_keep
    for T, plane in ((70, 0), (129, 3), (64, 5)):
        q, k = np.arange(T)[:, None], np.arange(T)[None, :]
        g, j = A.attn_groups(plane, T)
        gh, jh = hh.attn_group(plane, q, k, T)
        assert np.array_equal(g, gh) and np.array_equal(j, jh)
        rate = float(np.float32(0.2))
        want = dropout_keep(A.SEED, A.SITE, gh, jh, int(rate * 4294967296.0))
        got = A.keep_mask(1, 1, T, 0.2, plane0=plane)[0, 0].numpy() > 0
        assert np.array_equal(got, want)
        assert 0.7 < got.mean() < 0.9
    two = A.keep_mask(2, 2, 70, 0.2)
    assert torch.equal(A.keep_mask(1, 2, 70, 0.2, plane0=2), two[1:])


# ------------------------------------------------------------------ 2. the references against autograd and the oracle
def _dense_autograd(q, k, v, dout, B, H, T, vis, scale, keepc):
    """fp64 autograd of a dense masked softmax attention -> out, lse, dq, dk, dv (head layout [B][H][T][64])"""
    qh, kh, vh = (A.heads(x, B, H, T).clone().requires_grad_(True) for x in (q, k, v))
    w = float(np.float32(scale)) * (qh @ kh.transpose(-1, -2))
    if vis is not None:
        m = vis.to(F64)
        w = w * m - 1e4 * (1 - m)
    P = torch.softmax(w, -1)
    out = (P if keepc is None else P * keepc) @ vh
    (out * A.heads(dout, B, H, T)).sum().backward()
    wd = w.detach()
    mx = wd.max(-1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(wd - mx).sum(-1, keepdim=True))).squeeze(-1)
    return out.detach(), lse, qh.grad, kh.grad, vh.grad


PIN_CASES = [  # (B, H, T, L, spec, scale, rate, plane0)
    (2, 2, 70, 0, -1, 1.7, 0.0, 0), (2, 2, 70, 0, -1, 0.125, 0.2, 0), (1, 2, 70, 7, 8, 1.0, 0.2, 2), (2, 1, 48, 16, -1, 1.7, 0.0, 0),
    (1, 2, 45, 5, -3, 0.125, 0.2, 0), (1, 2, 40, 8, 0, 1.0, 0.0, 0), (1, 2, 40, 8, 4, 1.0, 0.0, 0), (1, 2, 40, 8, 7, 1.7, 0.2, 0),
    (1, 1, 50, 5, -2, 1.0, 0.0, 0),
]


@pytest.mark.parametrize('B,H,T,L,spec,scale,rate,plane0', PIN_CASES)
def test_references_against_dense_autograd(B, H, T, L, spec, scale, rate, plane0):
    q, k, v, dout = (R.normal((B * T, H * 64), 300 + i + T + L, 0.5 if i < 2 else 1.0) for i in range(4))
    keep = A.keep_mask(B, H, T, rate, plane0=plane0)
    c = A.drop_c(rate) if rate else 1.0
    ref = A.Ref(q, k, v, dout, B, H, T, L, spec, scale, keep, c)
    out, lse, dq, dk, dv = _dense_autograd(q, k, v, dout, B, H, T, A.token_mask(T, L, spec), scale, None if keep is None else keep * c)
    for name, want in (('out', A.rows(out)), ('lse', lse), ('dq', A.rows(dq)), ('dk', A.rows(dk)), ('dv', A.rows(dv))):
        val, mag = getattr(ref, name)
        assert _within(val, want, mag), name
        assert bool((mag >= val.abs() * (1 - 1e-9)).all()), name
    D, Dm = A.rowsum_D(dout, ref.out[0], B, H, T)
    assert _within(D, (A.heads(dout, B, H, T) * out).sum(-1), Dm) and _within(ref.D[0], D, Dm)
    assert float(ref.row_max.min()) > -1e4 + 104


def _oracle_attention(qh, kh, vh, B, H, nv, L, spec, dm):
    """the oracle's attention for view spec ``spec`` on head-layout tensors [B][H][T][64] -> out [B][H][T][64]; ``dm``: DropoutMasks"""
    from oracle import migt_oracle as mg

    def views(x, idx):
        return x.reshape(B, H, nv, L, 64)[:, :, idx]
    if spec <= -2:
        Sv, NS = -spec, nv // -spec
        sets = [[views(x, list(range(s * Sv, (s + 1) * Sv))) for s in range(NS)] for x in (kh, vh, qh)]
        if dm is None:
            outs = mg.compute_causal_block_multiend_attention(*sets)
        else:
            with mg.dropout_masks(dm):
                outs = mg.compute_causal_block_multiend_attention(*sets, layer=0)
        return torch.cat([o.reshape(B, H, Sv * L, 64) for o in outs], 2)
    Vc = nv if spec < 0 else min(spec, nv)
    full = dm.attn(0, 0, 'main') if dm is not None else None                      # one stream of nv views: [B][H][T][T] keep * c over absolute positions
    parts = []
    if Vc:
        idx = list(range(Vc))
        parts.append(mg.compute_causal_block_attention(views(kh, idx), views(vh, idx), views(qh, idx),
                                                       wmask=None if full is None else full[:, :, :Vc * L, :Vc * L]).reshape(B, H, Vc * L, 64))
    for e in range(Vc, nv):
        idx = list(range(Vc)) + [e]
        cols = torch.cat([torch.arange(Vc * L), torch.arange(e * L, (e + 1) * L)])
        wm = None if full is None else full[:, :, e * L:(e + 1) * L][:, :, :, cols]
        parts.append(mg.compute_causal_block_attention(views(kh, idx), views(vh, idx), views(qh, [e]), wmask=wm).reshape(B, H, L, 64))
    return torch.cat(parts, 2)


@pytest.mark.parametrize('B,H,nv,L,spec,scale,rate,b0', [
    (2, 2, 3, 4, -1, 1.0, 0.0, 0), (2, 2, 3, 4, -1, 1.7, 0.2, 0), (1, 2, 5, 4, 3, 1.0, 0.0, 0), (1, 2, 5, 4, 3, 0.125, 0.2, 1),
    (1, 2, 5, 4, 0, 1.0, 0.2, 0), (2, 2, 9, 4, -3, 1.0, 0.0, 0), (2, 2, 9, 4, -3, 1.7, 0.2, 1), (1, 1, 4, 4, -2, 1.0, 0.2, 0), (1, 1, 10, 3, -2, 1.0, 0.0, 0)])
def test_references_against_the_oracle(B, H, nv, L, spec, scale, rate, b0):
    """the oracle has no scale: it gets q scale, and autograd carries the factor back to dq"""
    from oracle.train_oracle import DropoutMasks
    T = nv * L
    q, k, v, dout = (R.normal((B * T, H * 64), 400 + i + T + nv, 0.5 if i < 2 else 1.0) for i in range(4))
    rate32 = float(np.float32(rate))
    NS = nv // -spec if spec <= -2 else 1
    dm = DropoutMasks(rate32, A.SEED, B, NS, nv // NS, L, H * 64, H, b0=b0) if rate else None
    keep = A.keep_mask(B, H, T, rate, plane0=b0 * H)
    c = A.drop_c(rate) if rate else 1.0
    ref = A.Ref(q, k, v, dout, B, H, T, L, spec, scale, keep, c)
    qh, kh, vh = (A.heads(x, B, H, T).clone().requires_grad_(True) for x in (q, k, v))
    out = _oracle_attention(qh * float(np.float32(scale)), kh, vh, B, H, nv, L, spec, dm)
    (out * A.heads(dout, B, H, T)).sum().backward()
    for name, want in (('out', out.detach()), ('dq', qh.grad), ('dk', kh.grad), ('dv', vh.grad)):
        val, mag = getattr(ref, name)
        assert _within(val, A.rows(want), mag), name


# ------------------------------------------------------------------ 3. precondition and calibration
@functools.lru_cache(maxsize=2)
def _ref(arm, name):
    case = (A.BF16_BY_NAME if arm == 'bf16' else A.F32_BY_NAME)[name]
    return A.reference(case, arm == 'bf16')


def _calibrate(arm, case):
    """worst restatement error per output on the GPU test's inputs (backward fed the reference's lse and D rounded to float32), and of the
    chain forward -> prep -> backward"""
    name, B, H, T, L, spec, scale, rate, kind = case
    bf16 = arm == 'bf16'
    unit = A.U16 if bf16 else A.U32
    q, k, v, dout = A.inputs(case, bf16)
    keep, c = A.case_keep(case)
    ref = _ref(arm, name)
    assert float(ref.row_max.min()) > -1e4 + 104, 'the precondition of the kernels: a masked weight is an exact zero'
    lse32, D32 = ref.lse[0].float(), ref.D[0].float()
    if bf16:
        out, lse = A.fwd_bf16(q, k, v, B, H, T, spec, scale, keep, c)
        D = A.prep_bf16(dout, ref.out[0].float().to(torch.bfloat16).float(), B, H, T)
        Dref = A.rowsum_D(dout, ref.out[0].float().to(torch.bfloat16).float(), B, H, T)
        dq, dk, dv = A.bwd_bf16(q, k, v, dout, lse32, D32, B, H, T, spec, scale, keep, c)
        cq, ck, cv = A.bwd_bf16(q, k, v, dout, lse, A.prep_bf16(dout, out, B, H, T), B, H, T, spec, scale, keep, c)
    else:
        out, lse = A.fwd_f32(q, k, v, B, H, T, L, spec, scale, keep, c)
        D = A.prep_f32(dout, ref.out[0].float(), B, H, T)
        Dref = A.rowsum_D(dout, ref.out[0].float(), B, H, T)
        dq, dk, dv = A.bwd_f32(q, k, v, dout, lse32, D32, B, H, T, L, spec, scale, keep, c)
        cq, ck, cv = A.bwd_f32(q, k, v, dout, lse, A.prep_f32(dout, out, B, H, T), B, H, T, L, spec, scale, keep, c)
    res = {'out': A.ratio(out, *ref.out, unit), 'lse': A.ratio(lse, *ref.lse, unit), 'D': A.ratio(D, *Dref, unit)}
    for n_, g, gc in (('dq', dq, cq), ('dk', dk, ck), ('dv', dv, cv)):
        res[n_] = max(A.ratio(g, *getattr(ref, n_), unit), A.ratio(gc, *getattr(ref, n_), unit))
    return res


_CAL = {}


@pytest.mark.parametrize('arm,name', [('f32', c[0]) for c in A.F32_CASES] + [('bf16', c[0]) for c in A.BF16_CASES])
def test_calibration_per_case(arm, name):
    case = (A.BF16_BY_NAME if arm == 'bf16' else A.F32_BY_NAME)[name]
    res = _calibrate(arm, case)
    _CAL[(arm, name)] = res
    print(f'basis {arm} [{name}]: ' + '  '.join(f'{k} {v:.3g}' for k, v in res.items()))
    assert all(np.isfinite(v) for v in res.values())


def test_calibration_covers_the_gpu_tests_constants():
    """c = 4 x the restatement's worst error over the cases, rounded up to a power of two, and the basis beside it in the GPU test's table is
    this run's (a float32 sum depends on how torch splits it: the table may sit one binade from this run's figure, never further).  The
    bf16 bases of the outputs that hold P stay within one decade across the cases, the large-score case included: the score term of the
    magnitude (module docstring of attention_kernels_ref.py) is what holds them together."""
    import test_hip_attention_kernels as G
    for arm, cases in (('f32', A.F32_CASES), ('bf16', A.BF16_CASES)):          # (whatever the per-case tests of this run did not leave)
        for case in cases:
            if (arm, case[0]) not in _CAL:
                _CAL[(arm, case[0])] = _calibrate(arm, case)
    worst = {}
    for (arm, name), res in _CAL.items():
        for k, v in res.items():
            worst[f'{arm} {k}'] = max(worst.get(f'{arm} {k}', 0.0), v)
    for k in sorted(worst):
        print(f'calibration {k}: restatement worst {worst[k]:.3g} units -> c = {_pow2_ceil(4 * worst[k]):g} (table: c = {G.C[k]:g}, basis {G.BASIS[k]:g})')
    assert set(worst) == set(G.C)
    for k, v in worst.items():
        assert G.C[k] == _pow2_ceil(4 * G.BASIS[k]), k
        assert _pow2_ceil(4 * v) <= 2 * G.C[k] and G.C[k] <= 2 * _pow2_ceil(4 * v), (k, v, G.C[k])
    for k in ('out', 'lse', 'dq', 'dk', 'dv'):
        per_case = [res[k] for (arm, name), res in _CAL.items() if arm == 'bf16']
        print(f'bf16 {k}: basis per case from {min(per_case):.3g} to {max(per_case):.3g}')
        assert max(per_case) <= 10 * min(per_case), (k, min(per_case), max(per_case))


# ------------------------------------------------------------------ 4. mutants
def _C(arm, out):
    import test_hip_attention_kernels as G
    return G.C[f'{arm} {out}'], (A.U16 if arm == 'bf16' else A.U32)


def _assert_rejected(arm, ref, mutant, outs, what):
    for o in outs:
        c, unit = _C(arm, o)
        r = A.ratio(getattr(mutant, o)[0], *getattr(ref, o), unit)
        print(f'mutant [{what}] {arm} {o}: {r:.3g} units (c = {c:g})')
        assert not r <= c, (what, arm, o, r, c)


def _case(arm, name):
    return (A.BF16_BY_NAME if arm == 'bf16' else A.F32_BY_NAME)[name]


ALL = ('out', 'dq', 'dk', 'dv')
STREAMS = {'f32': 'T576 L64 streams3x3 drop', 'bf16': '9 views streams3x3 drop'}
SCALED = {'f32': ['T144 L48 causal s1.7', 'T64 L64 causal s.125'], 'bf16': ['3 views causal s1.7', '2 views causal s.125']}


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_mutant_branch_view_sees_its_own_index_in_the_main_sequence(arm):
    case = _case(arm, STREAMS[arm])
    name, B, H, T, L, spec, *_ = case
    Sv, nv = -spec, T // L
    qv, kv = torch.arange(nv)[:, None], torch.arange(nv)[None, :]
    vm = torch.where(qv // Sv == 0, (kv // Sv == 0) & (kv % Sv <= qv % Sv), ((kv // Sv == 0) & (kv % Sv <= qv % Sv)) | (kv == qv))
    assert int((vm != A.view_matrix(nv, spec)).sum()) == (nv // Sv - 1) * Sv
    mutant = A.reference(case, arm == 'bf16', mut={'vis': A.token_mask(T, L, spec, views=vm)})
    _assert_rejected(arm, _ref(arm, name), mutant, ALL + ('lse',), 'ki <= qi for streams >= 1')


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_mutant_one_tile_visible_at_a_stream_boundary(arm):
    case = _case(arm, STREAMS[arm])
    name, B, H, T, L, spec, *_ = case
    vm = A.view_matrix(T // L, spec).clone()
    assert not bool(vm[3, 2])
    vm[3, 2] = True                                                              # the first view of stream 1 sees the last view of the sequence
    mutant = A.reference(case, arm == 'bf16', mut={'vis': A.token_mask(T, L, spec, views=vm)})
    _assert_rejected(arm, _ref(arm, name), mutant, ALL + ('lse',), 'one 64x64 tile visible')


def test_mutant_view_63_at_64_views():
    """the closed-form 64-bit masks at the limit: query view 63 left with itself alone (1ull << 63 lost, or bits 0 .. 62 lost with hi >= 64)"""
    case = _case('bf16', '64 views causal')
    name, B, H, T, L, spec, *_ = case
    vm = A.view_matrix(64, spec).clone()
    vm[63, :63] = False
    mutant = A.reference(case, True, mut={'vis': A.token_mask(T, L, spec, views=vm)})
    _assert_rejected('bf16', _ref('bf16', name), mutant, ALL + ('lse',), 'view 63 sees itself only')


@pytest.mark.parametrize('arm,name,other', [('f32', 'T256 L64 twin2 drop', 3), ('f32', 'T256 L64 twin3', 2), ('f32', 'T70 L7 twin8', 9), ('f32', 'T256 L64 twin0', 1),
                                            ('bf16', '5 views twin3 s1.7', 4), ('bf16', '5 views twin3 s1.7', 2), ('bf16', '5 views twin0', 1), ('bf16', '5 views twin4', 3)])
def test_mutant_twin_off_by_one(arm, name, other):
    case = _case(arm, name)
    _, B, H, T, L, spec, *_ = case
    mutant = A.reference(case, arm == 'bf16', mut={'vis': A.token_mask(T, L, other)})
    _assert_rejected(arm, _ref(arm, name), mutant, ALL + ('lse',), f'twin {spec} -> {other}')


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_mutant_scale_missing_in_one_place(arm):
    for name in SCALED[arm]:
        case = _case(arm, name)
        ref = _ref(arm, name)
        _assert_rejected(arm, ref, A.reference(case, arm == 'bf16', mut={'no_scale_dk': 1}), ('dk',), f'{name}: scale missing from dK')
        _assert_rejected(arm, ref, A.reference(case, arm == 'bf16', mut={'no_scale_dq': 1}), ('dq',), f'{name}: scale missing from dQ')
        _assert_rejected(arm, ref, A.reference(case, arm == 'bf16', mut={'no_scale_score': 1}), ALL + ('lse',), f'{name}: scale missing from the score')
        # and the other outputs of the first two are untouched: the factor sits in one place only
        m = A.reference(case, arm == 'bf16', mut={'no_scale_dk': 1})
        assert torch.equal(m.dq[0], ref.dq[0]) and torch.equal(m.dv[0], ref.dv[0])


@pytest.mark.parametrize('arm,name', [('f32', 'T70 none s1.7'), ('f32', 'T576 L64 streams3x3 drop'), ('bf16', '3 views causal s1.7'), ('bf16', '9 views streams3x3 drop')])
def test_mutant_D_term_dropped_for_one_wave(arm, name):
    case = _case(arm, name)
    mutant = A.reference(case, arm == 'bf16', mut={'no_D_rows': (32, 64)})
    _assert_rejected(arm, _ref(arm, name), mutant, ('dq', 'dk'), 'D dropped for queries 32 .. 63')


@pytest.mark.parametrize('arm,name', [('f32', 'T70 none drop'), ('f32', 'T256 L64 twin2 drop'), ('bf16', '9 views streams3x3 drop')])
def test_mutants_of_the_dropout(arm, name):
    case = _case(arm, name)
    _, B, H, T, L, spec, scale, rate, kind = case
    ref = _ref(arm, name)
    bf16 = arm == 'bf16'
    _assert_rejected(arm, ref, A.reference(case, bf16, mut={'dv_no_c': 1}), ('dv',), 'dV without 1 / (1 - rate)')
    _assert_rejected(arm, ref, A.reference(case, bf16, mut={'lse_after_dropout': 1}), ('lse',), 'lse after dropout')
    c = A.drop_c(rate)
    _assert_rejected(arm, ref, A.reference(case, bf16, keep=(A.keep_mask(B, H, T, rate, plane0=H), c)), ALL, 'drop_plane0 ignored')
    if T % 4:
        _assert_rejected(arm, ref, A.reference(case, bf16, keep=(A.keep_mask(B, H, T, rate, stride=T // 4), c)), ALL, 'group stride T // 4')
    else:
        assert torch.equal(A.keep_mask(B, H, T, rate, stride=T // 4), A.keep_mask(B, H, T, rate))


@pytest.mark.parametrize('arm,name', [('f32', 'T70 none s1.7'), ('f32', 'T384 L128 causal s1.7'), ('bf16', '1 view causal'), ('bf16', '5 views twin4')])
def test_mutant_heads_swapped(arm, name):
    ref = _ref(arm, name)
    for o in ALL:
        val, mag = getattr(ref, o)
        c, unit = _C(arm, o)
        swapped = torch.cat((val[:, 64:128], val[:, :64]), 1)
        assert A.rejects(swapped, val, mag, c, unit), (arm, name, o)


def test_mutant_unrounded_q_in_the_bf16_forward():
    """the forward's P from q scale log2 e WITHOUT its bf16 rounding, at the large-score case.  Against float64 this mutant is the better
    kernel: it differs from the real one by exactly the rounding whose cost the magnitude's score term states, so no comparison with float64
    can refuse it while accepting the kernel.  What it must not do is slip into the calibration: a restatement that skipped this rounding
    would put the basis of out several times, and of lse orders of magnitude, below what the kernel's stated arithmetic costs, and the
    kernel would then miss a constant derived from it.  (On the GPU a two-sided test does see it:
    test_hip_attention_kernels.py::test_bf16_forward_rounds_the_folded_q.)  Asserted: at |s| ~ 40 the rounding is the leading term of both outputs (it is what
    the table's constants are made of), and the magnitude without the score term would spread the bases of out over more than a decade."""
    case = _case('bf16', '4 views causal large')
    name, B, H, T, L, spec, scale, rate, kind = case
    q, k, v, dout = A.inputs(case, True)
    ref = _ref('bf16', name)
    smax = float((A.heads(q, B, H, T)[0, 0] @ A.heads(k, B, H, T)[0, 0].T).abs().max())
    assert smax > 25.0, smax
    out, lse = A.fwd_bf16(q, k, v, B, H, T, spec, scale)
    out_u, lse_u = A.fwd_bf16(q, k, v, B, H, T, spec, scale, unrounded_q=True)
    r, ru = A.ratio(out, *ref.out, A.U16), A.ratio(out_u, *ref.out, A.U16)
    l, lu = A.ratio(lse, *ref.lse, A.U16), A.ratio(lse_u, *ref.lse, A.U16)
    print(f'mutant [un-rounded q in the forward] bf16 out: {r:.3g} with the rounding, {ru:.3g} without; lse: {l:.3g}, {lu:.3g} (|s| <= {smax:.0f})')
    assert r > 4 * ru and l > 100 * lu
    c_out, c_lse = _C('bf16', 'out')[0], _C('bf16', 'lse')[0]
    assert _pow2_ceil(4 * ru) < c_out
    assert _pow2_ceil(4 * lu) < c_lse and l > _pow2_ceil(4 * lu), 'a constant calibrated without the rounding would refuse the restated kernel'
    # the plain rule (P's magnitude = P) at the same case and at the smallest scores of the list: more than a decade apart
    plain = A.reference(case, True, mut={'plain_magnitude': 1})
    small = _case('bf16', '2 views causal s.125')
    qs, ks, vs, _ = A.inputs(small, True)
    out_s, _ = A.fwd_bf16(qs, ks, vs, small[1], small[2], small[3], small[5], small[6])
    rp = A.ratio(out, *plain.out, A.U16)
    rs = A.ratio(out_s, *A.reference(small, True, mut={'plain_magnitude': 1}).out, A.U16)
    print(f'bf16 out under the plain rule: {rp:.3g} at |s| ~ 40 against {rs:.3g} at scale 0.125')
    assert rp > 10 * rs


# ------------------------------------------------------------------ 5. the host schedulers
def test_host_schedulers_sanitized(tmp_path):
    """tests/host/attn_schedulers.cpp: vf_attn_block_order is a permutation by descending weight with ties in index order, vf_attn_query_groups
    serves every view exactly once in at most 64 groups by descending weight (the size of the union of key views its views see, recomputed
    from vf_attn_visible; the struct holds no union of its own) — for nviews 1 .. 64, twin -32 .. 64, both by_key, vpb = 2.  Built for the host with AddressSanitizer and UBSan."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    exe = str(tmp_path / 'attn_schedulers')
    build = subprocess.run([hipcc, '-x', 'hip', '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                            '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(REPO, 'tests', 'host', 'attn_schedulers.cpp'), '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout.strip())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert '12416' in run.stdout and 'cells clean' in run.stdout
