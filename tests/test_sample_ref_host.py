"""CPU: the references of tests/sample_kernels_ref.py pinned against independent statements (the noise bit by bit and by its chi-square,
torch.topk, a float64 sort + cumsum, torch.log_softmax over the kept set), the usual mistakes rejected as mutants of the float32
restatement, the calibration of the GPU test's constants on its very inputs, the exemption cap on the reference alone, the argument
validation of the two entry points through ctypes and the host plumbing of ViewRenderer.sample.  No device is touched."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sample_kernels_ref as R


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


# ------------------------------------------------------------------ the noise
def _hash_py(seed, site, idx):
    """vf_dropout_hash in plain Python integers"""
    M = 0xFFFFFFFF
    h = (seed ^ (site * 0x9E3779B9)) & M
    h ^= idx & M
    h = (h * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h + (idx >> 32) * 0xC2B2AE35 + 0x27D4EB2F) & M
    h ^= h >> 16
    h = (h * 0x165667B1) & M
    h ^= h >> 15
    h = (h * 0xD3A2646C) & M
    return h ^ (h >> 16)


def _lowbias_py(x):
    M = 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M
    x ^= x >> 15
    x = (x * 0x846CA68B) & M
    return x ^ (x >> 16)


def test_the_noise_is_what_the_contract_says_bit_for_bit():
    from viewformer_amd import _hash
    assert _hash.SITE_SAMPLE == 0x5A0000 == R.SITE_SAMPLE
    for seed, rid, s, N in ((0, 0, 0, 5), (11, (2 << 32) | 77, 3, 130), (0xFFFFFFFF, (1 << 63) - 1, 65535, 64)):
        key = _hash_py(seed, 0x5A0000 + s, rid)
        assert _hash.sample_key(seed, rid, s) == key
        want = np.array([((_lowbias_py(n ^ key) >> 9) + 0.5) / 2.0 ** 23 for n in range(N)])
        u = _hash.sample_uniform(seed, rid, s, N)
        assert u.dtype == np.float64 and np.array_equal(u, want)
        assert np.array_equal(R.uniform(seed, [rid], s + 1, N)[0, s], want)          # the tests' own vectorised form
        assert np.all(u > 0) and np.all(u < 1)
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)            # exact in fp32 ...
        assert np.array_equal((np.float32(1) - u.astype(np.float32)).astype(np.float64), 1.0 - u)   # ... and so is 1 - u
        g = _hash.sample_gumbel(seed, rid, s, N)
        assert np.allclose(g, -np.log(-np.log(u)), rtol=1e-9, atol=1e-12) and np.array_equal(g, R.gumbel64(u))
    # the extremes of u: both finite, the largest key 16.6
    lo, hi = 0.5 * 2.0 ** -23, 1.0 - 2.0 ** -24
    assert abs(float(R.gumbel64(np.array([hi]))[0]) - 24 * math.log(2)) < 1e-6 and float(R.gumbel64(np.array([lo]))[0]) < -2.7
    with pytest.raises(ValueError):
        _hash.sample_key(0, 0, 65536)


def test_streams_of_different_samples_rows_and_seeds_differ():
    N = 256
    base = R.uniform(11, [5, 6, 5 | (1 << 32)], 4, N)
    assert not np.array_equal(base[0, 0], base[0, 1]) and not np.array_equal(base[0, 0], base[1, 0]) and not np.array_equal(base[0, 0], base[2, 0])
    other = R.uniform(12, [5], 1, N)
    assert not np.array_equal(base[0, 0], other[0, 0])
    for a, b in ((base[0, 0], base[0, 1]), (base[0, 0], base[1, 0]), (base[0, 0], other[0, 0]), (base[0, 0][:-1], base[0, 0][1:])):
        assert abs(float(np.corrcoef(a, b)[0, 1])) < 0.25                              # 256 values: |r| of independent streams is ~0.06
    # the definition's own correlations, on a long stream
    u = R.uniform(11, np.arange(64), 2, 4096)
    for a, b in ((u[:, 0], u[:, 1]), (u[:-1, 0], u[1:, 0]), (u[:, 0, :-1], u[:, 0, 1:])):
        assert abs(float(np.corrcoef(a.ravel(), b.ravel())[0, 1])) < 1e-2


# upper 99.9 % quantile of chi-square by Wilson-Hilferty (df ~ 100: within 0.1 of the exact value)
def _chi2_q999(df):
    return df * (1 - 2 / (9 * df) + 3.0902 * math.sqrt(2 / (9 * df))) ** 3


@pytest.mark.parametrize('seed', [11, 12, 13])
def test_reference_draws_follow_the_softmax(seed):
    """32 768 draws (4096 identical rows x S = 8, N = 128, T = 1) against the float64 soft-max; cells of expectation < 5 pooled"""
    N, rows, S = 128, 4096, 8
    z = (R.rng(500).standard_normal(N) * 2.0).astype(np.float32)
    ref = R.sample_ref(np.tile(z, (rows, 1)), 1.0, 0, 1.0, seed, np.arange(rows), S)
    p = np.exp(z.astype(np.float64) - z.max())
    p /= p.sum()
    obs = np.bincount(ref['idx'].ravel(), minlength=N).astype(np.float64)
    exp = p * rows * S
    small = exp < 5
    o = np.concatenate([obs[~small], [obs[small].sum()]])
    e = np.concatenate([exp[~small], [exp[small].sum()]])
    chi2, df = float(((o - e) ** 2 / e).sum()), o.size - 1
    print(f'seed {seed}: chi2 {chi2:.1f} at {df} degrees of freedom (99.9 %: {_chi2_q999(df):.1f})')
    assert chi2 <= _chi2_q999(df)
    # logp is the log of that soft-max at the draw
    assert np.allclose(ref['logp'], np.log(p)[ref['idx']], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ the reference against independent forms
def _by_definition(y, keep_k, p):
    """top-p straight from the definition, O(N^2): v* = the largest value v of the row with mass(v) >= p x total"""
    m = y[keep_k].max()
    e = np.where(keep_k, np.exp(y - m), 0.0)
    total = e.sum()
    ok = [v for v in np.unique(y[keep_k]) if e[y >= v].sum() >= p * total]
    return keep_k & (y >= max(ok))


@pytest.mark.parametrize('N', [1, 63, 65, 1026])
def test_reference_equals_independent_statements(N):
    rows = 9
    x, kinds, rid = R.inputs(rows, N, shift=0)
    z = x[:, :N].numpy()
    for T, top_k, top_p in ((1.0, 0, 1.0), (0.5, 2, 1.0), (2.0, 64, 0.9), (1.0, N, 0.5), (0.5, 0, 0.9), (2.0, N + 5, 1e-6), (1.0, 1, 0.9)):
        ref = R.sample_ref(z, T, top_k, top_p, 3, rid.numpy(), 2)
        y = torch.from_numpy(z).double() / T
        for r in range(rows):
            if kinds[r] == 'all_neg_inf':
                assert ref['idx'][r].tolist() == [-1, -1] and ref['kept'][r] == 0 and np.isnan(ref['thr'][r]) and np.isnan(ref['logp'][r]).all()
                continue
            fin = torch.isfinite(y[r])
            nf = int(fin.sum())
            keep = fin.clone()
            if 0 < top_k < nf:
                keep = y[r] >= torch.topk(y[r], top_k).values[-1]                      # ties at the k-th value are all kept
            if top_p < 1:
                keep = torch.from_numpy(_by_definition(y[r].numpy(), keep.numpy(), float(np.float32(top_p))))
            assert torch.equal(torch.from_numpy(ref['keep'][r]), keep), (N, kinds[r], T, top_k, top_p)
            assert ref['kept'][r] == int(keep.sum()) and ref['thr'][r] == float(y[r][keep].min())
            lsm = torch.log_softmax(y[r][keep], 0)
            pos = torch.cumsum(keep.long(), 0) - 1
            g = R.gumbel64(R.uniform(3, [int(rid[r])], 2, N))[0]
            for s in range(2):
                i = int(ref['idx'][r, s])
                assert bool(keep[i])
                assert abs(float(lsm[pos[i]]) - ref['logp'][r, s]) <= 1e-12 * (1 + abs(ref['logp'][r, s]))
                keys = torch.where(keep, y[r] + torch.from_numpy(g[s]), torch.tensor(-math.inf, dtype=torch.float64))
                assert i == int(torch.argmax(keys)) or float(keys[i]) == float(keys.max())
                assert ref['logp_mag'][r, s] >= abs(ref['logp'][r, s])


def test_reference_on_the_named_rows():
    N = 65
    eq = np.full((1, N), 1.5, np.float32)
    assert R.sample_ref(eq, 1.0, 0, 0.5)['kept'][0] == N                             # all-equal: the ties at v* are all kept
    assert R.sample_ref(eq, 1.0, 3, 1.0)['kept'][0] == N                             # ... and at the k-th value
    two = R.row_of('two_level', N, R.rng(0)).astype(np.float32)[None]
    ref = R.sample_ref(two, 1.0, 0, 0.9)
    assert ref['kept'][0] == 4 and ref['thr'][0] == 0.0
    # top_k = 1 on a unique maximum: the arg-max whatever the seed, logp = 0
    z = R.rng(1).standard_normal((5, N)).astype(np.float32)
    for seed in (0, 1, 99):
        ref = R.sample_ref(z, 0.5, 1, 1.0, seed, S=4)
        assert np.array_equal(ref['idx'], np.repeat(z.argmax(1)[:, None], 4, 1)) and np.all(ref['logp'] == 0) and np.all(ref['gap'] == np.inf)
    # equal keys: the lowest index (a kept set of equal logits under equal noise does not occur; the rule is pinned on the helper)
    assert R._first_argmax(np.array([[1.0, 3.0, 3.0, 2.0]])).tolist() == [1]


# ------------------------------------------------------------------ calibration of the GPU test's constants, and the cap
def _pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


_measured = {}


def _calibration():
    if not _measured:
        worst = [0.0, 0.0, 0.0]
        for case in R.all_cases():
            x, kinds, rid, ref = R.reference_for(case)
            r32 = R.restatement_for(case, x, rid, ref)
            dev = R.deviations(x[:, :case[1]].numpy(), ref, r32, case[5])
            worst = [max(a, b) for a, b in zip(worst, dev)]
        _measured.update(c_key=worst[0], c_mass=worst[1], c_logp=worst[2])
    return _measured


def test_the_gpu_tests_constants_are_calibrated_on_its_inputs():
    """basis = the float32 restatement's worst deviation from float64 on the GPU test's very inputs, in the unit of each tolerance;
    c = 4 x basis rounded up to a power of two.  The GPU test's TABLE must state both, to within one binade."""
    import test_hip_sample as G
    measured = _calibration()
    print({k: round(v, 3) for k, v in measured.items()})
    for k, b in measured.items():
        basis, c = G.TABLE[k]
        assert b > 0 and basis / 2 <= b <= basis * 2, (k, b, basis)
        assert c == _pow2_at_least(4 * basis), (k, basis, c)


@pytest.mark.parametrize('N', R.NS)
def test_the_restatement_passes_and_the_exempt_share_stays_within_the_cap(N):
    """on the reference alone: the exemptions at the TABLE's constants cover at most CAP of any one GPU test's cases — and the float32
    restatement, judged exactly as the kernel will be, passes"""
    import test_hip_sample as G
    cases = exempt = 0
    for case in R.cases(N):
        x, kinds, rid, ref = R.reference_for(case)
        r32 = R.sample_f32(x[:, :N].numpy(), case[3], case[4], case[5], case[7], rid.numpy(), case[2])
        j = R.judge(r32, ref, case[5], *G.CONSTANTS)
        assert j['errors'] == [], (case, j['errors'])
        cases, exempt = cases + j['cases'], exempt + j['exempt']
    print(f'N {N}: {exempt} of {cases} cases exempt')
    assert exempt <= R.CAP * cases


# ------------------------------------------------------------------ the mistakes
def test_the_usual_mistakes_are_rejected():
    import test_hip_sample as G
    rows, N, S, seed = 65, 65, 8, 11
    x, kinds, rid = R.inputs(rows, N, shift=0)
    z = x[:, :N].numpy()

    def run(T, top_k, top_p, mistake=None, row_ids=rid.numpy()):
        ref = R.sample_ref(z, T, top_k, top_p, seed, row_ids, S)
        got = R.sample_f32(z, T, top_k, top_p, seed, row_ids, S, mistake=mistake)
        return R.judge(got, ref, top_p, *G.CONSTANTS), got, ref
    for T, top_k, top_p in ((1.0, 0, 1.0), (2.0, 8, 0.9), (0.5, 2, 0.5), (2.0, 0, 0.9)):
        j, _, _ = run(T, top_k, top_p)
        assert j['errors'] == [] and j['exempt'] <= R.CAP * j['cases'], (T, top_k, top_p, j)
    j, _, _ = run(2.0, 8, 0.9, 'p_before_k')                    # the nucleus of the whole row is not the nucleus of its top 8
    assert any(e.startswith('kept') for e in j['errors'])
    j, got, ref = run(1.0, 3, 0.5, 'strict')                    # ties at the threshold dropped: the all-equal rows keep nothing but ...
    assert any(e.startswith('kept') for e in j['errors'])
    j, _, _ = run(2.0, 0, 0.9, 'temperature_last')              # the nucleus of z is not the nucleus of z / 2
    assert any(e.startswith('kept') for e in j['errors'])
    j, _, _ = run(1.0, 4, 1.0, 'logp_unfiltered')
    assert any(e.startswith('logp') for e in j['errors'])
    j, got, _ = run(1.0, 0, 1.0, 'no_s')
    assert any(e.startswith('idx') for e in j['errors']) and all(np.array_equal(got['idx'][:, 0], got['idx'][:, s]) for s in range(S))
    j, _, _ = run(1.0, 0, 1.0, 'row_position')
    assert any(e.startswith('idx') for e in j['errors'])
    j, _, _ = run(1.0, 0, 1.0, 'row_position', row_ids=np.arange(rows))      # (with row_id = the position the two coincide)
    assert j['errors'] == []
    # ties to the highest index: equal keys need equal logits AND equal noise words.  R.tie_rows builds such rows (two codes in different
    # lanes that share a 23-bit word and the logit 0): the keys tie bit for bit, the float64 gap is 0, and an exact tie is never exempt
    for Nt in (63, 1024, 1026):
        zt, rt, picks = R.tie_rows(Nt)
        assert len(picks) >= 4 and all((b - a) % 64 for _, a, b in picks)
        ref = R.sample_ref(zt, 1.0, 0, 1.0, 21, rt, 64)
        good = R.sample_f32(zt, 1.0, 0, 1.0, 21, rt, 64)
        bad = R.sample_f32(zt, 1.0, 0, 1.0, 21, rt, 64, mistake='tie_high')
        for i, (s, a, b) in enumerate(picks):
            assert ref['gap'][i, s] == 0 and ref['idx'][i, s] == a and good['keys'][i, s, a] == good['keys'][i, s, b]
            assert good['idx'][i, s] == a and bad['idx'][i, s] == b
        assert R.judge(good, ref, 1.0, *G.CONSTANTS)['errors'] == []
        j = R.judge(bad, ref, 1.0, *G.CONSTANTS)
        assert any(e.startswith('idx') for e in j['errors']), j
    # the judge itself: a draw outside the kept set, a wrong kept count, a NaN logp are all errors
    ref = R.sample_ref(z, 1.0, 2, 1.0, seed, rid.numpy(), S)
    good = R.sample_f32(z, 1.0, 2, 1.0, seed, rid.numpy(), S)
    live = int(np.argmax(~ref['empty'] & (ref['kept'] == 2) & (np.array(kinds) == 'spread')))
    bad = {k: v.copy() for k, v in good.items()}
    bad['idx'][live, 0] = int(np.argmin(z[live]))
    assert any('outside' in e for e in R.judge(bad, ref, 1.0, *G.CONSTANTS)['errors'])
    bad = {k: v.copy() for k, v in good.items()}
    bad['kept'][live] += 1
    assert any(e.startswith('kept') for e in R.judge(bad, ref, 1.0, *G.CONSTANTS)['errors'])
    bad = {k: v.copy() for k, v in good.items()}
    bad['logp'][live, 0] = np.nan
    assert any(e.startswith('logp') for e in R.judge(bad, ref, 1.0, *G.CONSTANTS)['errors'])
    # the pad: a read past N wins the row
    assert R.sample_ref(x.numpy(), 1.0, 1, 1.0, seed, rid.numpy(), 1)['idx'][0, 0] >= N


def test_inputs_have_the_properties_the_gpu_test_names():
    for N in R.NS:
        x, kinds, rid = R.inputs(65, N, shift=0)
        by = {k: kinds.index(k) for k in R.KINDS}
        z = x[:, :N]
        assert bool((x[:, N:] == 3e38).all()) and len(set(rid.tolist())) == 65 and int(rid.max()) >> 32 == 2
        assert bool(torch.isinf(z[by['all_neg_inf']]).all()) and bool(torch.isinf(z[by['neg_inf_entries']]).any()) == (N > 1)
        assert bool(torch.isfinite(z[by['neg_inf_entries']]).any())
        assert float(z[by['all_equal']].min()) == float(z[by['all_equal']].max())
        assert int((z[by['two_level']] == 0).sum()) == len(R.two_level_positions(N)) == min(4, N)
        if N > 1:
            assert bool((z[by['ascending']][1:] > z[by['ascending']][:-1]).all()) and bool((z[by['descending']][1:] < z[by['descending']][:-1]).all())
            assert float(z[by['flat']].std()) < 0.02
        if N >= 1024:
            assert float(z[by['spread']].max() - z[by['spread']].min()) > 100
    got = {(c[0], c[2], c[3], c[6]) for c in R.all_cases()}
    assert {c[0] for c in got} == set(R.ROWS) and {c[1] for c in got} == set(R.SS) and {c[2] for c in got} == set(R.TS) and {c[3] for c in got} == {False, True}
    for N in R.NS:
        assert {(c[4], c[5]) for c in R.cases(N)} == {(k, p) for k in R.top_ks(N) for p in R.TOP_PS}
        assert {(c[5], c[6]) for c in R.cases(N)} == {(p, l) for p in R.TOP_PS for l in (False, True)}      # every top_p meets both layouts
        assert {(c[4], c[6]) for c in R.cases(N)} == {(k, l) for k in R.top_ks(N) for l in (False, True)}


# ------------------------------------------------------------------ argument validation, no device
def _rows(lib, x=4096, rows=8, N=1000, ld=1000, T=1.0, top_k=0, top_p=1.0, seed=0, row_id=4096, S=2, idx=4096, logp=4096, kept=4096, thr=4096):
    ptr = lambda v: None if v is None else ctypes.c_void_p(v)          # never dereferenced: validation happens before any launch
    return lib.vf_sample_rows_f32(ptr(x), rows, N, ld, T, top_k, top_p, seed, ptr(row_id), S, ptr(idx), ptr(logp), ptr(kept), ptr(thr), None)


def test_entry_points_validate_their_arguments_without_a_device(lib):
    assert _rows(lib, x=None) == -1 and _rows(lib, idx=None) == -1
    assert _rows(lib, ld=999) == -1
    assert _rows(lib, T=0.0) == -1 and _rows(lib, T=-1.0) == -1 and _rows(lib, T=math.inf) == -1 and _rows(lib, T=math.nan) == -1
    assert _rows(lib, top_p=0.0) == -1 and _rows(lib, top_p=-0.5) == -1 and _rows(lib, top_p=math.nan) == -1
    assert _rows(lib, top_k=-1) == -1
    assert _rows(lib, S=0) == -1 and _rows(lib, S=65536) == -1
    assert _rows(lib, N=0, ld=0) == -1 and _rows(lib, rows=-1) == -1
    assert _rows(lib, N=65537, ld=65537) == -2
    assert _rows(lib, rows=0) == 0 and _rows(lib, rows=0, S=65535, N=65536, ld=65536, top_p=math.inf, logp=None, kept=None, thr=None, row_id=None) == 0
    P = ctypes.c_void_p
    d = P(4096)
    assert lib.vf_sample_views_f32(d, 0, 64, 8, d, None) == 0
    assert lib.vf_sample_views_f32(None, 4, 64, 8, d, None) == -1 and lib.vf_sample_views_f32(d, 4, 64, 8, None, None) == -1
    assert lib.vf_sample_views_f32(d, -1, 64, 8, d, None) == -1 and lib.vf_sample_views_f32(d, 4, 0, 8, d, None) == -1
    assert lib.vf_sample_views_f32(d, 4, 64, 0, d, None) == -1 and lib.vf_sample_views_f32(d, 4, 64, 65536, d, None) == -1
    assert lib.vf_abi_version() == 20                                                  # the additions are additive


def test_ops_refuse_cpu_tensors_and_unknown_outputs(lib):
    from viewformer_amd import ops, _lib
    with pytest.raises(_lib.VfError):
        ops.sample_rows(torch.zeros(4, 16), 4, 16)
    with pytest.raises(_lib.VfError):
        ops.sample_rows(torch.zeros(4, 16), 4, 16, row_id=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.sample_rows(torch.zeros(4, 16), 4, 16, want=())
    with pytest.raises(ValueError):
        ops.sample_rows(torch.zeros(4, 16), 4, 16, want=('logits',))
    with pytest.raises(_lib.VfError):
        ops.sample_views(torch.zeros(8, 2), 2, 4, 2)


# ------------------------------------------------------------------ host plumbing of ViewRenderer.sample
from render_fakes import Cfg as _Cfg, FakeCache as _FakeCache, FakeCodebook as _FakeCodebook, FakeModel as _FakeModel  # noqa: F401


def _renderer():
    from viewformer_amd.render import ViewRenderer
    r = ViewRenderer(_FakeModel(), _FakeCodebook())
    r.cache = _FakeCache()
    r.transform = torch.from_numpy(R.rng(7).standard_normal((2, 1, 7)).astype(np.float32))
    r._decode = lambda flat, keep_decoded=False: (flat[:, :4, :4, None].expand(-1, 4, 4, 3).to(torch.uint8), None)   # the decoder needs the device
    return r


def test_sample_walks_whole_views_with_their_numbers():
    from viewformer_amd.render import query_poses
    q = torch.from_numpy(R.rng(8).standard_normal((2, 8, 7)).astype(np.float32))
    r = _renderer()
    kw = dict(temperature=0.7, top_k=5, top_p=0.9, seed=3)
    one = r.sample(q, n_samples=3, return_codes=True, **kw)
    assert r.transformer.calls == [((2, 8, 7), 3, 0, kw)]
    assert tuple(one['generated_images'].shape) == (2, 8, 3, 4, 4, 3) and tuple(one['log_likelihood'].shape) == (2, 8, 3)
    assert set(one) == {'generated_images', 'log_likelihood', 'generated_codes', 'token_log_prob', 'kept'}
    assert set(r.sample(q)) == {'generated_images', 'log_likelihood'}
    want = query_poses(q, r.transform)                                               # the cameras reach the model in the context's frame
    assert torch.equal(one['token_log_prob'], one['generated_codes'].float() + want[..., 0].view(2, 8, 1, 1, 1))
    r2 = _renderer()
    parts = r2.sample(q, n_samples=3, max_views_per_call=3, return_codes=True, **kw)
    assert [(c[0][1], c[2]) for c in r2.transformer.calls] == [(3, 0), (3, 3), (2, 6)]      # every chunk is told its first view's number
    for k in one:
        assert torch.equal(one[k], parts[k]), k
    # N = 0: one call for the empty tensors, nothing to decode
    from viewformer_amd.render import ViewRenderer
    r3 = ViewRenderer(_FakeModel(), _FakeCodebook())
    r3.cache, r3.transform = _FakeCache(), None
    empty = r3.sample(q[:, :0], n_samples=2)
    assert r3.transformer.calls == [((2, 0, 7), 2, 0, dict(temperature=1.0, top_k=0, top_p=1.0, seed=0))]
    assert tuple(empty['generated_images'].shape) == (2, 0, 2, 32, 32, 3) and empty['generated_images'].dtype == torch.uint8
    assert tuple(empty['log_likelihood'].shape) == (2, 0, 2)


def test_sample_refusals_on_the_host():
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer
    q = torch.zeros((2, 4, 7))
    with pytest.raises(RuntimeError):
        ViewRenderer(_FakeModel(), _FakeCodebook()).sample(q)                        # no context
    r = _renderer()
    with pytest.raises(ValueError):
        r.sample(q[:1])                                                              # another batch size
    with pytest.raises(ValueError):
        r.sample(torch.zeros((2, 4, 6)))
    with pytest.raises(ValueError):
        r.sample(torch.zeros((2, 7)))
    with pytest.raises(ValueError):
        r.sample(q, max_views_per_call=0)
    m = MIGT(MIGTConfig(sequence_size=3, n_layer=1))
    with pytest.raises(TypeError):
        m.sample_from_context(_FakeCache(), q)                                       # not a ContextCache of prefill_context
