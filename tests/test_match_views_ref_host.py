"""CPU: the references of tests/match_views_ref.py pinned against independent statements (torch's float64 log_softmax + gather + sum, the
in-order sum of tests/test_hip_score.py), the derived bound on the float32 restatement, the mistakes it must tell apart, the new symbol in
the binding and in the cross-compiled library, the entry point's refusals through ctypes (they return before any launch) and the host
side of ViewRenderer.match.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

import match_views_ref as R


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


_cache = {}


def _case(c):
    """inputs, float64 reference and float32 restatement of a case: computed once, shared, left unchanged"""
    k = R.case_id(c)
    if k not in _cache:
        inp = R.inputs(c)
        _cache[k] = (inp, R.reference(inp, c), R.restated_f32(inp, c))
    return _cache[k]


def _scene(codes, b):
    return codes[b if codes.shape[0] > 1 else 0]


def test_case_list_covers_the_values_and_plants_the_codes():
    want = dict(L={1, 3, 64, 65}, V={1, 7, 128, 1024}, pad={0, 5}, B={1, 3}, M={1, 2, 5}, P={1, 63, 64, 65, 257},
                stride={'shared', 'dense', 'gap'}, spread={0.05, 3.0, 60.0})
    for k, v in want.items():
        assert {c[k] for c in R.CASES} == v, k
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:
        inp = _case(c)[0]
        V = c['V']
        flat = inp['codes'].reshape(-1)
        for v in (0, V - 1, -1, V, R.I32_MIN, R.I32_MAX):
            assert (flat == v).any(), (R.case_id(c), v)
        assert np.isneginf(inp['logits'][inp['inf_row'], :V]).all() and np.isneginf(inp['lse'][inp['inf_row']])
        assert (inp['logits'][:, V:] == np.float32(R.PAD_FILL)).all()
        assert inp['codes'].shape == (1 if c['stride'] == 'shared' else c['B'], c['P'], c['L'])
        assert R.scene_stride(c) in (0, c['P'] * c['L'], c['P'] * c['L'] + 3)


@pytest.mark.parametrize('c', R.CASES, ids=R.case_id)
def test_reference_equals_torch_float64_log_softmax_gather_sum(c):
    """on the elements whose codes all lie in [0, V) and whose rows are not the -inf row.  The reference takes the float32 lse it is given,
    log_softmax forms its own in float64: they differ by that one rounding per token, sum_t 2^-24 |lse_t| (plus float64 noise)."""
    inp, (ll, mag, acc), _ = _case(c)
    L, V, B, M, P = c['L'], c['V'], c['B'], c['M'], c['P']
    lp = torch.log_softmax(torch.from_numpy(inp['logits'][:, :V].astype(np.float64)), -1).view(B, M, L, V)
    lse_abs = np.abs(inp['lse'].astype(np.float64)).reshape(B, M, L)
    checked = 0
    for b in range(B):
        cb = torch.from_numpy(_scene(inp['codes'], b).astype(np.int64))                    # [P, L]
        inside = ((cb >= 0) & (cb < V)).all(1).numpy()
        for m in range(M):
            g = lp[b, m].gather(1, cb.clamp(0, V - 1).t()).sum(0).numpy()                 # [L, P] summed over tokens
            want_acc = (torch.from_numpy(inp['idx']).view(B, M, L)[b, m][None, :] == cb).double().mean(1).numpy()
            assert np.array_equal(acc[b, m], want_acc)
            if (b * M + m) * L <= inp['inf_row'] < (b * M + m + 1) * L:
                continue                                                               # the view with the -inf row: NaN or -inf
            tol = R.U * lse_abs[b, m].sum() + 1e-12 * (1.0 + mag[b, m])
            assert (np.abs(ll[b, m] - g)[inside] <= tol[inside]).all(), (b, m)
            assert np.isneginf(ll[b, m][~inside]).all()                                # an out-of-range code: -inf, whatever the rest
            checked += int(inside.sum())
    assert checked > 0


@pytest.mark.parametrize('c', R.CASES, ids=R.case_id)
def test_reference_and_restatement_equal_the_in_order_sum_of_the_score_tests(c):
    """tests/test_hip_score.py::_in_order_sum is the statement vf_score_views_f32 is held to: s = x_0; s = s + x_t.  The restatement is
    that sum of the float32 token log-probabilities, bit for bit; the reference is the same sum in float64."""
    import test_hip_score as G
    inp, (ll, _, _), (ll32, _) = _case(c)
    L, V, B, M, P = c['L'], c['V'], c['B'], c['M'], c['P']
    z = inp['logits'].reshape(B, M, L, -1)
    for dt, want in ((torch.float32, ll32), (torch.float64, ll)):
        x = torch.empty((B, M, P, L), dtype=dt)
        for b in range(B):
            cb = torch.from_numpy(_scene(inp['codes'], b).astype(np.int64))
            ok = (cb >= 0) & (cb < V)
            for m in range(M):
                zt = torch.from_numpy(z[b, m, :, :V]).to(dt).t()[cb.clamp(0, V - 1), torch.arange(L)[None, :]]       # [P, L]
                x[b, m] = torch.where(ok, zt - torch.from_numpy(inp['lse']).view(B, M, L)[b, m].to(dt)[None, :], torch.tensor(-np.inf, dtype=dt))
        s = G._in_order_sum(x.view(-1, L)).view(B, M, P)
        if dt == torch.float32:
            assert torch.equal(R.bits(s), R.bits(want)), 'float32 restatement'
        else:
            assert np.array_equal(s.numpy(), want, equal_nan=True), 'float64 reference'


@pytest.mark.parametrize('c', R.CASES, ids=R.case_id)
def test_restatement_stays_within_the_derived_bound(c):
    inp, (ll, mag, acc), (ll32, acc32) = _case(c)
    r = R.worst_ratio(ll32, ll, mag, c['L'])
    print(f'{R.case_id(c)}: worst {r:.4f} x gamma_L x magnitude')
    assert r <= 1.0, (R.case_id(c), r)
    assert np.array_equal(acc32, acc.astype(np.float32))                               # hits / L rounds once, as the float64 quotient does
    assert np.isfinite(ll).any() and np.isneginf(ll).any()


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_mistake_differs_from_the_restatement_on_the_case_list(mistake):
    """on EVERY case where the mistake computes something else (R.applies), and there is such a case"""
    hit = 0
    for c in R.CASES:
        inp, _, (ll32, acc32) = _case(c)
        bad_ll, bad_acc = R.restated_f32(inp, c, mistake=mistake)
        differs = not (torch.equal(R.bits(bad_ll), R.bits(ll32)) and torch.equal(R.bits(bad_acc), R.bits(acc32)))
        if R.applies(mistake, c):
            assert differs, (mistake, R.case_id(c))
            hit += 1
    assert hit >= 2, mistake


def test_the_chain_mistakes_leave_the_derived_bound_or_the_bits():
    """pairwise and sum-then-subtract are close to the truth (they are sums too): it takes the bits to tell them from the chain, which is
    why the GPU test asks for bits; swapping P and M, another photo, clamping and the ignored stride are far outside the bound"""
    for mistake in ('swap_pm', 'next_photo', 'clamp', 'ignore_stride'):
        far = 0
        for c in R.CASES:
            if R.applies(mistake, c):
                inp, (ll, mag, _), _ = _case(c)
                far += not R.worst_ratio(R.restated_f32(inp, c, mistake=mistake)[0], ll, mag, c['L']) <= 1.0
        assert far >= 1, mistake


# ------------------------------------------------------------------ the symbol and its refusals, no device
def test_symbol_is_bound_and_exported(lib):
    from viewformer_amd import _lib
    assert 'vf_match_views_f32' in _lib.EXPORTS
    assert len(_lib.EXPORTS['vf_match_views_f32'][1]) == 14
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'vf_match_views_f32')
    assert lib.vf_abi_version() == 20


def _call(lib, logits=4096, ld=1024, lse=4096, idx=4096, codes=4096, stride=0, B=2, M=3, P=5, L=64, V=1024, ll=4096, acc=4096):
    ptr = lambda x: None if x is None else ctypes.c_void_p(x)          # never dereferenced: validation happens before any launch
    return lib.vf_match_views_f32(ptr(logits), ld, ptr(lse), ptr(idx), ptr(codes), stride, B, M, P, L, V, ptr(ll), ptr(acc), None)


def test_entry_point_validates_its_arguments_without_a_device(lib):
    BAD, UNSUPPORTED = -1, -2
    for k in ('logits', 'lse', 'codes', 'll'):
        assert _call(lib, **{k: None}) == BAD, k
    assert _call(lib, idx=None) == BAD                                                 # accuracy without idx
    for k in ('B', 'M', 'P'):
        assert _call(lib, **{k: -1}) == BAD, k
    assert _call(lib, L=0) == BAD and _call(lib, L=-64) == BAD and _call(lib, V=0) == BAD and _call(lib, V=-1) == BAD
    assert _call(lib, ld=1023) == BAD
    assert _call(lib, stride=5 * 64 - 1) == BAD and _call(lib, stride=1) == BAD and _call(lib, stride=-1) == BAD
    # refusals come first: a bad argument is refused even where nothing would be launched
    assert _call(lib, B=0, ld=1023) == BAD and _call(lib, P=0, logits=None) == BAD
    # no-ops
    assert _call(lib, B=0) == 0 and _call(lib, M=0) == 0 and _call(lib, P=0) == 0
    assert _call(lib, P=0, stride=0) == 0 and _call(lib, M=0, stride=5 * 64) == 0 and _call(lib, M=0, idx=None, acc=None) == 0
    # the grid: B M ceil(P / 256) workgroups in one dimension
    assert _call(lib, B=1 << 20, M=1 << 12) == UNSUPPORTED
    assert _call(lib, B=1 << 16, M=1 << 14, P=512) == UNSUPPORTED
    assert _call(lib, B=1 << 40, M=1 << 40) == UNSUPPORTED


def test_ops_match_views_refuses_on_the_host(lib):
    from viewformer_amd import ops, _lib
    z, lse, idx = torch.zeros(6 * 4, 8), torch.zeros(24), torch.zeros(24, dtype=torch.int64)
    codes = torch.zeros((2, 5, 4), dtype=torch.int32)
    with pytest.raises(_lib.VfError):
        ops.match_views(z, lse, idx, codes, 2, 3, 5, 4, 8)                             # host tensors: no CPU route


# ------------------------------------------------------------------ host side of ViewRenderer.match
from render_fakes import Cfg as _Cfg, FakeCache as _FakeCache, FakeCodebook as _FakeCodebook, FakeModel as _FakeModel  # noqa: F401


def _renderer():
    from viewformer_amd.render import ViewRenderer
    r = ViewRenderer(_FakeModel(), _FakeCodebook())
    r.cache = _FakeCache()
    r.transform = None
    return r


def test_match_refusals_and_empty_shapes_on_the_host():
    from viewformer_amd.render import ViewRenderer
    q = torch.zeros((2, 4, 7))
    codes = torch.zeros((2, 5, 8, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ViewRenderer(_FakeModel(), _FakeCodebook()).match(q, codes=codes)            # no context
    r = _renderer()
    imgs = torch.zeros((2, 5, 32, 32, 3), dtype=torch.uint8)
    bad = [dict(), dict(images=imgs, codes=codes), dict(codes=codes.float()), dict(codes=codes.bool()), dict(codes=codes[:, :, :4]),
           dict(codes=codes.view(2, 5, 64)), dict(codes=torch.zeros((3, 5, 8, 8), dtype=torch.int32)), dict(images=imgs[0]),
           dict(images=torch.zeros((3, 5, 32, 32, 3), dtype=torch.uint8))]
    for kw in bad:
        with pytest.raises(ValueError):
            r.match(q, **kw)
    for qq in (q[:1], q[..., :6], q[0]):
        with pytest.raises(ValueError):
            r.match(qq, codes=codes)
    assert r.transformer.calls == []                                                 # every refusal came before the model was asked
    # M = 0 and P = 0; a shared photo set reaches the model as it is
    out = r.match(q[:, :0], codes=codes[:1])
    assert r.transformer.calls == [((2, 0, 7), (1, 5, 8, 8), {})]
    assert tuple(out['log_likelihood'].shape) == (2, 5, 0) and tuple(out['best_photo'].shape) == (2, 0)
    assert out['best_camera'].dtype == torch.int64 and out['best_camera'].tolist() == [[-1] * 5] * 2
    out = r.match(q, codes=codes[:, :0], max_views_per_call=3)
    assert [c[0] for c in r.transformer.calls[1:]] == [(2, 3, 7), (2, 1, 7)]          # whole views, P not chunked
    assert tuple(out['log_likelihood'].shape) == (2, 0, 4) and tuple(out['accuracy'].shape) == (2, 0, 4)
    assert tuple(out['best_camera'].shape) == (2, 0) and out['best_photo'].tolist() == [[-1] * 4] * 2
    assert tuple(out['predicted_codes'].shape) == (2, 4, 8, 8)
