"""CPU: the references of the mean-view kernel (tests/mix_kernels_ref.py) pinned against independent statements — torch's float64
soft-max, torch.topk and the O(N^2) definition of top-p —, the claim the feature rests on (the mean of the codebook over the SAMPLER's
draws converges to it), the usual mistakes rejected, the GPU test's constant calibrated on its own inputs, and the argument validation of
vf_mix_rows_f32 through ctypes.  No device is touched.  The reference-side tests pass on any tree; the validation tests need the symbol."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mix_kernels_ref as M
import sample_kernels_ref as R

F64 = np.float64


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _rows_of_every_kind(N, seed=0):
    x, kinds, _ = R.inputs(len(R.KINDS), N, 0, seed)
    return x[:, :N].numpy(), kinds


# ------------------------------------------------------------------ the reference against independent statements
@pytest.mark.parametrize('N', [1, 63, 128, 1024])
def test_reference_without_filters_is_the_softmax_times_the_codebook(N):
    z, kinds = _rows_of_every_kind(N)
    E = M.codebook(32, N)[:, :N].numpy()
    for T in R.TS:
        ref = M.mix_ref(z, E, T)
        want = torch.softmax(torch.from_numpy(z).double() / float(np.float32(T)), -1) @ torch.from_numpy(E).double().T
        live = ~ref['empty']
        assert live.sum() == len(kinds) - 1 and np.isnan(ref['out'][~live]).all()
        assert np.allclose(ref['out'][live], want.numpy()[live], rtol=1e-12, atol=1e-13)
        assert (ref['mag'][live] >= np.abs(ref['out'][live])).all()
        assert np.allclose(ref['p'][live].sum(1), 1.0, rtol=1e-13)


def _keep_by_definition(y, top_k, top_p):
    """one row, float64: torch.topk for the k-th value (ties kept), then the O(N^2) definition of the nucleus on what is left"""
    fin = np.isfinite(y)
    keep = fin.copy()
    if top_k > 0 and top_k < fin.sum():
        vk = torch.topk(torch.from_numpy(y), top_k).values[-1].item()
        keep &= y >= vk
    if top_p < 1.0:
        e = np.where(keep, np.exp(y - y[fin].max()), 0.0)
        best = None
        for v in y[keep]:                                                          # the largest value whose upper mass reaches top_p x total
            if e[y >= v].sum() >= top_p * e.sum() and (best is None or v > best):
                best = v
        keep &= y >= best
    return keep


@pytest.mark.parametrize('N', [63, 128])
def test_reference_with_filters_equals_topk_and_the_quadratic_top_p(N):
    z, kinds = _rows_of_every_kind(N, seed=1)
    E = M.codebook(32, N)[:, :N].numpy().astype(F64)
    for T, top_k, top_p in ((1.0, 5, 1.0), (0.5, 0, 0.9), (2.0, 16, 0.5), (1.0, N + 5, 1e-6), (2.0, 2, 0.9)):
        ref = M.mix_ref(z, E, T, top_k, top_p)
        for r, kind in enumerate(kinds):
            if kind == 'all_neg_inf':
                assert ref['kept'][r] == 0 and np.isnan(ref['out'][r]).all()
                continue
            y = z[r].astype(F64) / float(np.float32(T))
            keep = _keep_by_definition(y, top_k, float(np.float32(top_p)))
            assert np.array_equal(keep, ref['keep'][r]), (kind, T, top_k, top_p)
            p = torch.softmax(torch.from_numpy(np.where(keep, y, -math.inf)), -1).numpy()
            assert np.array_equal(p == 0, ~keep)
            assert np.allclose(ref['out'][r], E @ p, rtol=1e-12, atol=1e-13), (kind, T, top_k, top_p)
            assert np.array_equal(M.keep_from_count(z[r:r + 1], ref['kept'][r:r + 1])[0], keep)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_the_mean_of_the_samplers_draws_converges_to_the_reference(seed):
    """the claim the feature rests on: E[:, idx] averaged over ``sample_ref``'s draws (the sampler's definition, 32 768 of them) lands
    within 5 standard errors of ``mix_ref`` in every feature — the variance taken from the reference distribution"""
    N, D, S, T, top_k, top_p = 64, 32, 32768, 2.0, 16, 0.9
    z = np.stack([R.row_of('normal4', N, R.rng(50)), R.row_of('flat', N, R.rng(51))]).astype(np.float32)
    E = M.codebook(D, N)[:, :N].numpy().astype(F64)
    ref = M.mix_ref(z, E, T, top_k, top_p)
    assert 1 < ref['kept'][0] <= 16 and 1 < ref['kept'][1] <= 16
    idx = R.sample_ref(z, T, top_k, top_p, seed, np.array([3, (1 << 32) + 9]), S)['idx']
    for r in range(2):
        mean = E[:, idx[r]].mean(1)
        var = (ref['p'][r] * E ** 2).sum(1) - ref['out'][r] ** 2
        se = np.sqrt(var / S)
        dev = np.abs(mean - ref['out'][r]) / se
        print(f'seed {seed} row {r}: worst {dev.max():.2f} standard errors')
        assert (dev <= 5.0).all(), (r, dev.max())


# ------------------------------------------------------------------ the constant, the restatement, the mistakes
def _pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


_measured = {}


def _calibration():
    if not _measured:
        worst = 0.0
        for case in M.all_cases():
            x, E, kinds, ref = M.reference_for(case)
            rows, N, D, T, top_k, top_p, padded, shift = case
            r32 = M.mix_f32(x[:, :N].numpy(), E[:, :N].numpy(), T, top_k, top_p)
            if np.array_equal(r32['kept'], ref['kept']):                            # (a nucleus decided the other way in float32: another set)
                ref_k = ref
            else:
                ref_k = M.mix_ref(x[:, :N].numpy(), E[:, :N].numpy(), T, top_k, top_p, keep=r32['keep'])
            w = M.worst_ratio(r32['out'], ref_k)
            assert math.isfinite(w), case
            worst = max(worst, w)
        _measured['c_out'] = worst
    return _measured


def test_the_gpu_tests_constant_is_calibrated_on_its_inputs():
    """basis = the float32 restatement's worst deviation from float64 on the GPU test's very inputs, each judged on its own kept set as
    the kernel will be; c = 4 x basis rounded up to a power of two.  The table must state both, to within one binade."""
    b = _calibration()['c_out']
    print(f'c_out: measured basis {b:.3f}, table {M.C_OUT}')
    basis, c = M.C_OUT
    assert b > 0 and basis / 2 <= b <= basis * 2, (b, basis)
    assert c == _pow2_at_least(4 * basis), (basis, c)


def test_the_exact_class_is_exact_in_the_restatement():
    for case in M.exact_cases():
        z, E, ref = M.exact_inputs(case)
        rows, N, D, T, top_k, top_p = case
        r32 = M.mix_f32(z.numpy(), E[:, :N].numpy(), T, top_k, top_p)
        assert (r32['kept'] == N).all()
        assert np.array_equal(r32['out'].astype(F64), ref['out']), case
        assert np.array_equal(ref['out'], E[:, :N].numpy().astype(F64).sum(1)[None].repeat(rows, 0) / N)


def test_top_k_1_is_the_codebook_column_in_the_restatement():
    N, D = 128, 32
    x, kinds, _ = R.inputs(9, N, 0)
    z, E = x[:, :N].numpy(), M.codebook(D, N)[:, :N].numpy()
    r32 = M.mix_f32(z, E, 0.5, 1, 1.0)
    for r, kind in enumerate(kinds):
        if kind in ('spread', 'flat', 'ascending', 'descending', 'normal4'):
            assert r32['kept'][r] == 1 and np.array_equal(r32['out'][r], E[:, int(z[r].argmax())])


def test_the_usual_mistakes_are_rejected():
    """each mutant leaves the bound of the GPU test, c x 2^-24 x magnitude, by orders of magnitude on rows of the case table"""
    N, D = 128, 32
    x, kinds, _ = R.inputs(len(R.KINDS), N, 0)
    z, E = x[:, :N].numpy(), M.codebook(D, N)[:, :N].numpy()
    c = M.C_OUT[1]
    where = dict(temperature_last=(0.5, 0, 0.9), unfiltered_sum=(1.0, 8, 1.0), p_before_k=(1.0, 64, 0.9), strict=(1.0, 2, 0.5),
                 tile_dropped=(1.0, 0, 1.0), E_transposed=(1.0, 0, 1.0))
    assert set(where) == set(M.MISTAKES)
    for mistake, (T, top_k, top_p) in where.items():
        zz = np.where(np.isfinite(z), np.floor(z), z) if mistake == 'strict' else z      # whole numbers: ties at the threshold
        ref = M.mix_ref(zz, E, T, top_k, top_p)
        got = M.mix_mutant(zz, E, T, top_k, top_p, mistake)
        live = ~ref['empty']
        got[~live] = math.nan
        w = M.worst_ratio(got, ref)
        print(f'{mistake}: {w:.3g} x 2^-24 x magnitude')
        assert w > 1000 * c, (mistake, w)
        # ... and the reference itself, through the same comparison, passes
        assert M.worst_ratio(ref['out'].copy(), ref) == 0.0


def test_the_case_table_has_the_values_the_issue_names():
    cases = M.all_cases()
    assert {c[1] for c in cases} == {1, 63, 64, 65, 128, 1024} and {c[2] for c in cases} == {32, 256}
    assert {c[0] for c in cases} == {1, 3, 15, 16, 17, 33} and {c[3] for c in cases} == {0.5, 1.0, 2.0} and {c[6] for c in cases} == {False, True}
    for N in M.NS:
        assert {(c[4], c[5]) for c in M.cases(N)} == {(k, p) for k in (0, 1, 2, 64, N, N + 5) for p in (1.0, 0.9, 0.5, 1e-6)}
        assert {c[0] for c in M.cases(N)} == set(M.ROWS) and {c[2] for c in M.cases(N)} == set(M.DS) and {c[3] for c in M.cases(N)} == set(M.TS)
    kinds = set()
    for c in cases:
        kinds |= set(M.inputs_for(c)[2])
    assert kinds == set(R.KINDS)
    x, E, _ = M.inputs_for(cases[0])
    assert bool((x[:, cases[0][1]:] == 3e38).all()) and bool(torch.isnan(E[:, cases[0][1]:]).all())


# ------------------------------------------------------------------ argument validation, no device
def _mix(lib, x=4096, rows=8, N=1000, ld=1000, T=1.0, top_k=0, top_p=1.0, E=4096, D=256, ldE=1000, out=4096, ldo=256, kept=4096, thr=4096):
    ptr = lambda v: None if v is None else ctypes.c_void_p(v)          # never dereferenced: validation happens before any launch
    return lib.vf_mix_rows_f32(ptr(x), rows, N, ld, T, top_k, top_p, ptr(E), D, ldE, ptr(out), ldo, ptr(kept), ptr(thr), None)


def test_the_entry_point_validates_its_arguments_without_a_device(lib):
    assert _mix(lib, x=None) == -1 and _mix(lib, E=None) == -1 and _mix(lib, out=None) == -1
    assert _mix(lib, rows=-1) == -1 and _mix(lib, N=0, ld=0, ldE=0) == -1
    assert _mix(lib, ld=999) == -1 and _mix(lib, ldE=999) == -1 and _mix(lib, ldo=255) == -1
    assert _mix(lib, T=0.0) == -1 and _mix(lib, T=-1.0) == -1 and _mix(lib, T=math.inf) == -1 and _mix(lib, T=math.nan) == -1
    assert _mix(lib, top_p=0.0) == -1 and _mix(lib, top_p=-0.5) == -1 and _mix(lib, top_p=math.nan) == -1
    assert _mix(lib, top_k=-1) == -1
    assert _mix(lib, N=1025, ld=1025, ldE=1025) == -2
    assert _mix(lib, D=48, ldo=48) == -2 and _mix(lib, D=16, ldo=16) == -2 and _mix(lib, D=288, ldo=288) == -2
    assert _mix(lib, rows=0) == 0 and _mix(lib, rows=0, N=1024, ld=1024, ldE=1024, D=32, ldo=32, top_p=math.inf, kept=None, thr=None) == 0
    assert _mix(lib, rows=0, N=1025, ld=1025, ldE=1025) == -2 and _mix(lib, rows=0, T=0.0) == -1      # refusals come first
    assert lib.vf_abi_version() == 20                                                  # the addition is additive


def test_the_symbol_is_exported_and_ops_refuse_host_tensors(lib):
    from viewformer_amd import ops, _lib
    assert 'vf_mix_rows_f32' in _lib.EXPORTS and hasattr(lib, 'vf_mix_rows_f32')
    assert ops.MIX_ROWS_PER_GROUP == M.ROWS_PER_GROUP
    assert ops.mix_rows_supported(256, 1024) and ops.mix_rows_supported(32, 128) and ops.mix_rows_supported(32, 64)
    assert not ops.mix_rows_supported(256, 1025) and not ops.mix_rows_supported(48, 64) and not ops.mix_rows_supported(288, 64)
    assert not ops.mix_rows_supported(0, 64) and not ops.mix_rows_supported(32, 0)
    z, E = torch.zeros(4, 64), torch.zeros(32, 64)
    with pytest.raises(_lib.VfError):
        ops.mix_rows(z, 4, 64, E, 32)
    with pytest.raises(ValueError):
        ops.mix_rows(z, 4, 64, E, 32, want=())
    with pytest.raises(ValueError):
        ops.mix_rows(z, 4, 64, E, 32, want=('idx',))
