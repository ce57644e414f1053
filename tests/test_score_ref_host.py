"""CPU: the references of tests/score_kernels_ref.py pinned against independent statements (torch's float64 log_softmax, cross_entropy and
Categorical entropy, the oracle's logits), the mistakes they must reject, the calibration of the GPU test's constants, the argument
validation of the three entry points through ctypes, and the host plumbing of ViewRenderer.score.  No device is touched."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import score_kernels_ref as S


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


# ------------------------------------------------------------------ the float64 references against independent statements
def test_references_equal_torch_float64():
    for rows, N in ((5, 1), (7, 65), (33, 1024)):
        z = S.normal((rows, N), 10 + N, 3.0).double()
        tgt = torch.from_numpy(S.rng(11 + N).integers(0, N, size=rows))
        st = S.score_stats(z, tgt)
        lp = torch.log_softmax(z, -1)
        assert torch.equal(st['idx'][0], z.argmax(-1))
        assert torch.equal(st['max_logit'][0], z.max(-1).values)
        assert torch.allclose(st['lse'][0], torch.logsumexp(z, -1), rtol=1e-14, atol=1e-14)
        assert torch.allclose(st['target_logit'][0] - st['lse'][0], -F.cross_entropy(z, tgt, reduction='none'), rtol=1e-13, atol=1e-13)
        assert torch.allclose(st['entropy'][0], torch.distributions.Categorical(logits=z).entropy(), rtol=1e-12, atol=1e-13)
        assert torch.allclose(S.token_log_prob(z, tgt)[0], lp.gather(1, tgt[:, None])[:, 0], rtol=1e-13, atol=1e-13)
        for k in ('lse', 'entropy'):
            assert bool((st[k][1] >= st[k][0].abs()).all())                       # a magnitude bounds its value
    # ties to the lowest index; targets outside the codes; -inf codes; a row of nothing but -inf
    z = torch.tensor([[1.0, 3.0, 3.0, -math.inf], [-math.inf] * 4], dtype=torch.float64)
    st = S.score_stats(z, torch.tensor([-1, 4]))
    assert st['idx'][0].tolist() == [1, 0] and st['target_logit'][0].tolist() == [-math.inf, -math.inf]
    assert st['lse'][0][1] == -math.inf and math.isnan(st['entropy'][0][1])
    assert abs(float(st['entropy'][0][0]) - float(torch.distributions.Categorical(logits=z[0, :3]).entropy())) < 1e-14


def test_references_equal_the_oracles_logits_statistics():
    """the statistics of the fp64 oracle's last-view logits, stated with torch on the oracle's own output"""
    from oracle import migt_oracle as mg
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.weights import make_migt_weights
    cfg = MIGTConfig(n_embeddings=128, n_head=2, d_model=128, n_layer=1, token_image_size=8, sequence_size=3, pose_multiplier=0.2)
    sd = make_migt_weights(cfg, seed=3, std=0.05)
    g = S.rng(5)
    ids = torch.from_numpy(g.integers(0, 128, size=(1, 3, 8, 8)))
    ids[:, -1] = cfg.n_embeddings
    poses = torch.from_numpy(g.standard_normal((1, 3, 7)).astype(np.float32))
    lg = mg.migt_forward(sd, cfg, ids, poses, dtype=torch.float64)['logits'][0, -1].reshape(64, 128)
    tgt = torch.from_numpy(g.integers(0, 128, size=64))
    st = S.score_stats(lg, tgt)
    lp = torch.log_softmax(lg, -1)
    assert torch.allclose(st['target_logit'][0] - st['lse'][0], lp.gather(1, tgt[:, None])[:, 0], rtol=1e-12, atol=1e-12)
    assert torch.allclose(st['entropy'][0], -(lp.exp() * lp).sum(-1), rtol=1e-11, atol=1e-12)
    assert torch.equal(st['idx'][0], lg.argmax(-1))


# ------------------------------------------------------------------ calibration of the GPU test's constants
def _pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(x))


def _fused_basis():
    worst = {'lse': 0.0, 'entropy': 0.0}
    for K, N in S.FUSED_KN:
        for M in S.FUSED_M:
            h, wte, tgt, _ = S.fused_inputs(M, K, N)
            z = S.fused_logits_f32(h, wte)
            ref, got = S.score_stats(z, tgt), S.fused_score_f32(z.numpy(), tgt.numpy())
            assert S.mismatches(got['idx'], ref['idx'][0]) == 0 and S.mismatches(got['max_logit'], ref['max_logit'][0]) == 0
            assert S.mismatches(got['target_logit'], ref['target_logit'][0]) == 0
            for k in worst:
                worst[k] = max(worst[k], S.worst_ratio(torch.from_numpy(got[k]), *ref[k]))
    return worst


def _rows_basis():
    worst = {'lse': 0.0, 'entropy': 0.0}
    for N in S.ROWS_N:
        for kind in S.ROWS_KINDS:
            x, tgt = S.rows_inputs(5, N, kind)
            z = x[:, :N]
            ref, got = S.score_stats(z, tgt), S.rows_score_f32(z.numpy(), tgt.numpy())
            for k in ('idx', 'max_logit', 'target_logit'):
                assert S.mismatches(got[k], ref[k][0]) == 0, (N, kind, k)
            for k in worst:
                bad, fin = S.split_special(torch.from_numpy(got[k]), ref[k][0])
                assert bad == 0, (N, kind, k)
                if bool(fin.any()):
                    worst[k] = max(worst[k], S.worst_ratio(torch.from_numpy(got[k])[fin], ref[k][0][fin], ref[k][1][fin]))
    return worst


def test_the_gpu_tests_constants_are_calibrated_on_its_inputs():
    """basis = the float32 restatement's worst error against float64 in units of 2^-24 x magnitude on the GPU test's very inputs;
    c = 4 x basis rounded up to a power of two.  The GPU test's TABLE must state both, to within one binade."""
    import test_hip_score as G
    measured = {}
    for name, w in (('fused', _fused_basis()), ('rows', _rows_basis())):
        for k, b in w.items():
            measured[f'{name} {k}'] = b
    print({k: round(v, 3) for k, v in measured.items()})
    for k, b in measured.items():
        basis, c = G.TABLE[k]
        assert b > 0 and basis / 2 <= b <= basis * 2, (k, b, basis)
        assert c == _pow2_at_least(4 * basis), (k, basis, c)


# ------------------------------------------------------------------ the mistakes
def test_the_usual_mistakes_are_rejected():
    import test_hip_score as G
    K, N, M = 128, 1024, 65
    h, wte, tgt, kinds = S.fused_inputs(M, K, N)
    z = S.fused_logits_f32(h, wte)
    ref = S.score_stats(z, tgt)
    good = S.fused_score_f32(z.numpy(), tgt.numpy())
    for k in ('lse', 'entropy'):
        assert S.worst_ratio(torch.from_numpy(good[k]), *ref[k]) <= G.TABLE[f'fused {k}'][1]

    def far(out, k):
        return S.rejects(torch.from_numpy(out[k]), *ref[k], G.TABLE[f'fused {k}'][1])
    bad = S.fused_score_f32(z.numpy(), tgt.numpy(), mistake='no_rescale')              # the sums keep terms relative to a stale maximum
    assert far(bad, 'lse') and far(bad, 'entropy')
    bad = S.fused_score_f32(z.numpy(), tgt.numpy(), mistake='drop_tile')
    assert far(bad, 'lse') and S.mismatches(bad['idx'], ref['idx'][0]) > 0             # 'ascending' rows lose their maximum with it
    bad = S.fused_score_f32(z.numpy(), tgt.numpy(), mistake='entropy_sign')
    assert far(bad, 'entropy')
    bad = S.fused_score_f32(z.numpy(), tgt.numpy(), mistake='wrong_row')
    assert S.mismatches(bad['target_logit'], ref['target_logit'][0]) > 0
    bad = S.fused_score_f32(z.numpy(), tgt.numpy(), mistake='tie_high')
    tie_rows = [m for m, kd in enumerate(kinds) if kd.startswith('tie_')]
    assert tie_rows and all(int(bad['idx'][m]) != int(ref['idx'][0][m]) for m in tie_rows)
    assert S.mismatches(good['idx'], ref['idx'][0]) == 0
    # one tile per wave: dropping a wave's codes
    h, wte, tgt, _ = S.fused_inputs(33, 128, 128)
    z = S.fused_logits_f32(h, wte)
    bad = S.fused_score_f32(z.numpy(), tgt.numpy(), mistake='drop_tile')
    assert S.rejects(torch.from_numpy(bad['lse']), *S.score_stats(z, tgt)['lse'], G.TABLE['fused lse'][1])
    # the row kernel's pad: a read past N wins the row
    x, tgt = S.rows_inputs(5, 63, 'normal')
    assert S.mismatches(S.rows_score_f32(x.numpy(), tgt.numpy())['max_logit'], S.score_stats(x[:, :63], tgt)['max_logit'][0]) == 5


def test_fused_inputs_have_the_properties_the_gpu_test_names():
    for K, N in S.FUSED_KN:
        h, wte, tgt, kinds = S.fused_inputs(65, K, N)
        z = S.fused_logits_f32(h, wte)
        st = S.score_stats(z, tgt)
        idx, mx = st['idx'][0], st['max_logit'][0]
        by = {kd: kinds.index(kd) for kd in S.FUSED_KINDS}
        assert float(z[by['spread']].max() - z[by['spread']].min()) > 110                       # tails underflow in float32
        assert int(idx[by['ascending']]) == N - 1 and int(idx[by['max_last']]) == N - 1 and int(idx[by['descending']]) == 0
        assert int(idx[by['tie_lanes']]) == 3 and float(z[by['tie_lanes'], 4]) == float(mx[by['tie_lanes']])
        assert int(idx[by['tie_waves']]) == 7 and float(z[by['tie_waves'], 7 + N // 4]) == float(mx[by['tie_waves']])
        assert int(idx[by['tie_tiles']]) == 5 and int((z[by['tie_tiles']] == mx[by['tie_tiles']]).sum()) == 2
        assert tgt[:8].tolist() == [0, 31, 32, N // 4 - 1, N // 4, N - 1, -1, N]


# ------------------------------------------------------------------ argument validation, no device
def _fused(lib, h=4096, h16=0, ldh=768, w=4096, M=64, K=768, N=1024, target=4096, idx=4096, mx=4096, lse=4096, tl=4096, ent=4096):
    ptr = lambda x: None if x is None else ctypes.c_void_p(x)          # never dereferenced: validation happens before any launch
    return lib.vf_lmhead_score_bf16(ptr(h), h16, ldh, ptr(w), M, K, N, ptr(target), ptr(idx), ptr(mx), ptr(lse), ptr(tl), ptr(ent), None)


def _rows(lib, x=4096, rows=8, N=1000, ld=1000, target=4096, idx=4096, mx=4096, lse=4096, tl=4096, ent=4096):
    ptr = lambda v: None if v is None else ctypes.c_void_p(v)
    return lib.vf_logits_score_f32(ptr(x), rows, N, ld, ptr(target), ptr(idx), ptr(mx), ptr(lse), ptr(tl), ptr(ent), None)


def test_entry_points_validate_their_arguments_without_a_device(lib):
    none = dict(idx=None, mx=None, lse=None, tl=None, ent=None)
    assert _fused(lib, h=None) == -1 and _fused(lib, w=None) == -1
    assert _fused(lib, **none) == -1                                                   # no output requested
    assert _fused(lib, target=None) == -1                                              # target_logit without targets
    assert _fused(lib, M=-1) == -1 and _fused(lib, K=-768) == -1 and _fused(lib, N=-1) == -1 and _fused(lib, ldh=512) == -1
    assert _fused(lib, N=1000) == -2 and _fused(lib, K=256, ldh=256) == -2
    assert _fused(lib, ldh=770) == -2 and _fused(lib, h16=1, ldh=772) == -2            # rows are read as vectors
    assert _fused(lib, M=0) == 0
    assert _fused(lib, M=0, N=1000) == -2                                              # ... but an unsupported shape is still refused
    assert _rows(lib, x=None) == -1 and _rows(lib, **none) == -1 and _rows(lib, target=None) == -1
    assert _rows(lib, rows=-1) == -1 and _rows(lib, N=0) == -1 and _rows(lib, ld=999) == -1
    assert _rows(lib, rows=0) == 0
    P = ctypes.c_void_p
    d = P(4096)
    assert lib.vf_score_views_f32(d, d, d, d, d, 0, 64, d, d, d, d, None) == 0
    assert lib.vf_score_views_f32(d, d, d, d, d, 4, 0, d, d, d, d, None) == -1
    assert lib.vf_score_views_f32(d, d, d, d, None, 4, 64, d, d, d, d, None) == -1
    assert lib.vf_score_views_f32(d, d, d, d, d, -1, 64, d, d, d, d, None) == -1


def test_ops_refuse_cpu_tensors_and_unknown_outputs(lib):
    from viewformer_amd import ops, _lib
    assert ops.lmhead_score_supported(768, 1024) and ops.lmhead_score_supported(128, 128)
    assert not ops.lmhead_score_supported(256, 1024) and not ops.lmhead_score_supported(768, 1000)
    with pytest.raises(_lib.VfError):
        ops.lmhead_score_bf16(torch.zeros(4, 128), torch.zeros(128 * 128, dtype=torch.bfloat16), 4, 128, 128, want=('lse',))
    with pytest.raises(_lib.VfError):
        ops.logits_score(torch.zeros(4, 16), 4, 16, want=('lse',))
    with pytest.raises(_lib.VfError):
        ops.logits_score(torch.zeros(4, 16), 4, 16, target=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.logits_score(torch.zeros(4, 16), 4, 16, want=())
    with pytest.raises(ValueError):
        ops.logits_score(torch.zeros(4, 16), 4, 16, want=('logits',))
    with pytest.raises(ValueError):
        ops.logits_score(torch.zeros(4, 16), 4, 16, want=('target_logit',))


# ------------------------------------------------------------------ host plumbing of ViewRenderer.score
from render_fakes import Cfg as _Cfg, FakeCache as _FakeCache, FakeCodebook as _FakeCodebook, FakeModel as _FakeModel  # noqa: F401


def _renderer(transform=True):
    from viewformer_amd.render import ViewRenderer
    r = ViewRenderer(_FakeModel(), _FakeCodebook())
    r.cache = _FakeCache()
    g = S.rng(7)
    r.transform = torch.from_numpy(g.standard_normal((2, 1, 7)).astype(np.float32)) if transform else None
    return r


def test_score_walks_whole_views_and_broadcasts_one_photo():
    from viewformer_amd.render import query_poses
    g = S.rng(8)
    q = torch.from_numpy(g.standard_normal((2, 8, 7)).astype(np.float32))
    codes = torch.from_numpy(g.integers(0, 128, size=(2, 8, 8, 8))).to(torch.int32)
    r = _renderer()
    one = r.score(q, codes=codes)
    assert r.transformer.calls == [((2, 8, 7), (2, 8, 8, 8), {})]
    # the cameras reach the model in the context's frame
    want = query_poses(q, r.transform)
    assert torch.equal(one['token_log_prob'], codes.float() + want[..., 0].view(2, 8, 1, 1))
    r2 = _renderer()
    r2.fused_score = False
    parts = r2.score(q, codes=codes, max_views_per_call=3)
    assert [c[0][1] for c in r2.transformer.calls] == [3, 3, 2] and [c[1][1] for c in r2.transformer.calls] == [3, 3, 2]
    assert all(c[2] == dict(fused=False) for c in r2.transformer.calls)
    for k in one:
        assert torch.equal(one[k], parts[k]), k
    # one photo per scene: every chunk gets the same single code map, and the result is that of the photo repeated
    r3 = _renderer()
    single = r3.score(q, codes=codes[:, :1], max_views_per_call=4)
    assert [c[1] for c in r3.transformer.calls] == [(2, 1, 8, 8), (2, 1, 8, 8)]
    rep = _renderer().score(q, codes=codes[:, :1].expand(2, 8, 8, 8).contiguous())
    for k in single:
        assert torch.equal(single[k], rep[k]), k
    # photos are resized and encoded once, whatever the chunking
    r4 = _renderer(transform=False)
    imgs = torch.from_numpy(g.integers(0, 128, size=(2, 8, 32, 32, 3)).astype(np.uint8))
    r4.score(q, images=imgs, max_views_per_call=2)
    assert r4.codebook.encoded == 16 and len(r4.transformer.calls) == 4
    # N = 0
    r5 = _renderer()
    r5.score(q[:, :0], codes=codes[:, :0])
    assert r5.transformer.calls == [((2, 0, 7), (2, 0, 8, 8), {})]


def test_score_refusals_on_the_host():
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer
    g = S.rng(9)
    q = torch.zeros((2, 4, 7))
    codes = torch.zeros((2, 4, 8, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ViewRenderer(_FakeModel(), _FakeCodebook()).score(q, codes=codes)            # no context
    r = _renderer()
    with pytest.raises(ValueError):
        r.score(q)                                                                   # neither photos nor codes
    with pytest.raises(ValueError):
        r.score(q, images=torch.zeros((2, 4, 32, 32, 3), dtype=torch.uint8), codes=codes)
    with pytest.raises(ValueError):
        r.score(q, codes=codes.float())
    with pytest.raises(ValueError):
        r.score(q, codes=codes[:, :3])                                               # 3 photos for 4 cameras
    with pytest.raises(ValueError):
        r.score(q[:1], codes=codes)                                                  # another batch size
    with pytest.raises(ValueError):
        r.score(q, codes=codes.view(2, 4, 64))                                       # token maps are [t, t], as the model requires
    with pytest.raises(ValueError):
        r.score(torch.zeros((2, 4, 6)), codes=codes)
    with pytest.raises(ValueError):
        r.score(q, images=torch.zeros((2, 3, 32, 32, 3), dtype=torch.uint8))
    m = MIGT(MIGTConfig(sequence_size=3, n_layer=1))
    with pytest.raises(TypeError):
        m.score_from_context(_FakeCache(), q, codes)                                 # not a ContextCache of prefill_context
