"""GPU: sampling novel views (csrc/sample_rows.hip, MIGT.sample_from_context, ViewRenderer.sample) — the row kernel against the float64
reference of tests/sample_kernels_ref.py (pinned on the CPU by tests/test_sample_ref_host.py), its determinism contract, its footprint,
the in-order log-likelihood chain, then the model and the renderer.

Exact class: kept / thr without top-p, membership of every draw in the reference's kept set, top_k = 1 against ops.argmax_rows, the
named rows.  Rounded class (idx, kept / thr under top-p, logp) with the exemptions of sample_kernels_ref.judge, which are statements about
the float64 reference; at most 0.5 % of a test's (row, sample) cases may be exempt.  ``TABLE`` holds one (basis, c) per constant: basis =
the worst deviation of the float32 CPU restatement of the kernel from float64 on these very inputs, as the host file measures it, c = 4 x
basis rounded up to a power of two — never a figure taken from the kernel."""
import ctypes
import itertools
import types

import numpy as np
import pytest
import torch

import sample_kernels_ref as R
from conftest import parity_report
from framed import Frame

pytestmark = pytest.mark.gpu

# constant: (basis, c); test_sample_ref_host.py::test_the_gpu_tests_constants_are_calibrated_on_its_inputs
TABLE = {
    'c_key': (3.2, 16.0),           # x 2^-24 x (max |y| + max |g|): the gap below which a draw may differ
    'c_mass': (4.93, 32.0),         # x 2^-24: how close to top_p a normalised mass must lie for the nucleus to differ
    'c_logp': (1.6, 8.0),           # x 2^-24 x (|y_idx| + magnitude of lse)
}
CONSTANTS = tuple(TABLE[k][1] for k in ('c_key', 'c_mass', 'c_logp'))
OUT = ('idx', 'logp', 'kept', 'thr')
_worst = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        parity_report(test='sample_kernels', what=k, **_worst[k])


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f'{what}: {k} differs in its bits'


def _note(name, j):
    w = _worst.setdefault(name, dict(cases=0, exempt=0, worst_logp=0.0, c_key=CONSTANTS[0], c_mass=CONSTANTS[1], c_logp=CONSTANTS[2]))
    w['cases'] += j['cases']
    w['exempt'] += j['exempt']
    w['worst_logp'] = max(w['worst_logp'], j['worst_logp'])


def _run(dev, case, x, row_ids, want=OUT):
    from viewformer_amd import ops
    rows, N, S, T, top_k, top_p, padded, seed, shift = case
    xd = x.to(dev) if padded else x[:, :N].contiguous().to(dev)
    return ops.sample_rows(xd, rows, N, temperature=T, top_k=top_k, top_p=top_p, seed=seed, row_id=row_ids.to(dev), n_samples=S,
                           ld=N + R.PAD if padded else None, want=want)


# ------------------------------------------------------------------ the kernel against the reference
@pytest.mark.parametrize('N', R.NS)
def test_row_kernel_against_the_reference(dev, N):
    """every (top_k, top_p) of the lists at this N; rows 1 / 3 / 65, S 1 / 3 / 8, T 0.5 / 1 / 2, compact and padded rows (+3e38 in the
    pad: a read past N wins the row) walk with the case; rows of every kind of R.KINDS"""
    cases = exempt = 0
    for case in R.cases(N):
        x, kinds, rid, ref = R.reference_for(case)
        got = _run(dev, case, x, rid)
        assert got['idx'].dtype == torch.int64 and got['kept'].dtype == torch.int32 and tuple(got['idx'].shape) == (case[0], case[2])
        j = R.judge(got, ref, case[5], *CONSTANTS)
        print(f'{case}: {j["exempt"]} of {j["cases"]} exempt, logp worst {j["worst_logp"]:.3f} x 2^-24 x magnitude')
        assert j['errors'] == [], (case, j['errors'])
        _note(f'N {N}', j)
        cases, exempt = cases + j['cases'], exempt + j['exempt']
    assert exempt <= R.CAP * cases, f'{exempt} of {cases} cases exempt'


@pytest.mark.parametrize('N', R.NS)
def test_top_k_1_is_the_argmax_whatever_the_seed(dev, N):
    from viewformer_amd import ops
    x, kinds, rid = R.inputs(65, N, shift=0)
    z = x[:, :N]
    unique = ((z == z.max(1, keepdim=True).values).sum(1) == 1) & torch.isfinite(z.max(1).values)
    assert int(unique.sum()) >= 40
    xd = x.to(dev)
    am = ops.argmax_rows(xd, 65, N, ld=N + R.PAD)
    for seed, T, S in ((0, 1.0, 1), (1, 0.5, 3), (7, 2.0, 8), (123456789, 1.0, 3)):
        got = ops.sample_rows(xd, 65, N, temperature=T, top_k=1, seed=seed, row_id=rid.to(dev), n_samples=S, ld=N + R.PAD, want=OUT)
        u = unique.to(dev)
        assert torch.equal(got['idx'][u], am[u][:, None].expand(-1, S)), (seed, T)
        assert bool((got['logp'][u] == 0).all()) and bool((got['kept'][u] == 1).all())
        assert torch.equal(got['thr'][u], (z.max(1).values / T).to(dev)[u])


@pytest.mark.parametrize('N', R.NS)
def test_the_named_rows(dev, N):
    """the all-equal row at top_p = 0.5 keeps all N (ties at v* are kept); the two-level row at top_p = 0.9 keeps its zeros; every draw
    comes from the kept set"""
    from viewformer_amd import ops
    g = R.rng(5)
    x = torch.from_numpy(np.stack([R.row_of('all_equal', N, g), R.row_of('two_level', N, g)]).astype(np.float32)).to(dev)
    for T in R.TS:
        a = ops.sample_rows(x, 2, N, temperature=T, top_p=0.5, seed=3, n_samples=8, want=OUT)
        assert int(a['kept'][0]) == N and float(a['thr'][0]) == 1.5 / T
        b = ops.sample_rows(x, 2, N, temperature=T, top_p=0.9, seed=3, n_samples=8, want=OUT)
        pos = R.two_level_positions(N)
        assert int(b['kept'][1]) == len(pos) and float(b['thr'][1]) == 0.0
        assert set(b['idx'][1].tolist()) <= set(pos)
        c = ops.sample_rows(x, 2, N, temperature=T, top_k=3, seed=3, n_samples=8, want=OUT)      # ties at the k-th value
        assert int(c['kept'][0]) == N and int(c['kept'][1]) == len(pos)


@pytest.mark.parametrize('N', [63, 1024, 1026])
def test_on_equal_keys_the_lowest_index_wins(dev, N):
    """rows of R.tie_rows: two codes in different lanes share a noise word and the logit 0, every other code sits 40 below — the two
    best keys are equal bit for bit whatever the accuracy of the logarithms, and the draw must be the lower code.  This is the wave's
    butterfly (``oi < bi``).  The lane's own strict compare is not reached by an exact tie: no two codes of one lane (64 k apart) were
    found to share a noise word (see R.tie_rows), so that half of the rule is not asserted here."""
    from viewformer_amd import ops
    z, rid, picks = R.tie_rows(N)
    assert len(picks) >= 4
    ref = R.sample_ref(z, 1.0, 0, 1.0, 21, rid, 64)
    got = ops.sample_rows(torch.from_numpy(z).to(dev), len(picks), N, seed=21, row_id=torch.from_numpy(rid).to(dev), n_samples=64, want=OUT)
    for i, (s, a, b) in enumerate(picks):
        assert ref['gap'][i, s] == 0 and ref['idx'][i, s] == a
        assert int(got['idx'][i, s]) == a, (N, i, s, a, b, int(got['idx'][i, s]))
    j = R.judge(got, ref, 1.0, *CONSTANTS)
    assert j['errors'] == [], j['errors']
    assert j['exempt'] <= R.CAP * j['cases']
    # under top_k = 2 the kept set is exactly the tying pair (the third value sits 40 below): the same decision
    two = ops.sample_rows(torch.from_numpy(z).to(dev), len(picks), N, top_k=2, seed=21, row_id=torch.from_numpy(rid).to(dev), n_samples=64, want=OUT)
    assert bool((two['kept'] == 2).all()) and all(int(two['idx'][i, s]) == a for i, (s, a, b) in enumerate(picks))


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize('N', [65, 1024, 1026])
def test_a_rows_outputs_depend_on_nothing_but_the_row(dev, N):
    from viewformer_amd import ops
    rows, T, top_k, top_p, seed = 65, 0.5, 64, 0.9, 11
    x, kinds, rid = R.inputs(rows, N, shift=3)
    xd, xc, rd = x.to(dev), x[:, :N].contiguous().to(dev), rid.to(dev)
    kw = dict(temperature=T, top_k=top_k, top_p=top_p, seed=seed)
    full = ops.sample_rows(xd, rows, N, row_id=rd, n_samples=8, ld=N + R.PAD, want=OUT, **kw)
    # two launches with the same arguments; compact rows
    _same_bits(ops.sample_rows(xd, rows, N, row_id=rd, n_samples=8, ld=N + R.PAD, want=OUT, **kw), full, 'second launch')
    _same_bits(ops.sample_rows(xc, rows, N, row_id=rd, n_samples=8, want=OUT, **kw), full, 'compact')
    # row 40 alone, with its row_id
    alone = ops.sample_rows(xc[40:41], 1, N, row_id=rd[40:41].contiguous(), n_samples=8, want=OUT, **kw)
    _same_bits(alone, {k: v[40:41] for k, v in full.items()}, 'row 40 alone')
    # S = 3 against the first three samples of S = 8
    three = ops.sample_rows(xc, rows, N, row_id=rd, n_samples=3, want=OUT, **kw)
    _same_bits(three, dict(idx=full['idx'][:, :3], logp=full['logp'][:, :3], kept=full['kept'], thr=full['thr']), 'S = 3 of 8')
    # every combination of optional outputs
    for n in range(1, 5):
        for want in itertools.combinations(OUT, n):
            got = ops.sample_rows(xc, rows, N, row_id=rd, n_samples=8, want=want, **kw)
            assert tuple(got) == want
            _same_bits(got, {k: full[k] for k in want}, f'want {want}')
    # row_id = NULL is the row's number
    _same_bits(ops.sample_rows(xc, rows, N, n_samples=8, want=OUT, **kw),
               ops.sample_rows(xc, rows, N, row_id=torch.arange(rows, dtype=torch.int64, device=dev), n_samples=8, want=OUT, **kw), 'row_id NULL')
    # another seed changes at least a quarter of the draws of the nearly uniform row; another row_id and another s likewise
    flat = kinds.index('flat')
    a = ops.sample_rows(xc[flat:flat + 1], 1, N, seed=1, n_samples=64)['idx']
    b = ops.sample_rows(xc[flat:flat + 1], 1, N, seed=2, n_samples=64)['idx']
    c = ops.sample_rows(xc[flat:flat + 1], 1, N, seed=1, row_id=torch.tensor([1 << 32], device=dev), n_samples=64)['idx']
    assert int((a != b).sum()) >= 16 and int((a != c).sum()) >= 16 and len(set(a[0].tolist())) >= 16


# ------------------------------------------------------------------ footprint, and the chain
@pytest.mark.parametrize('rows,N,S', [(7, 1026, 3), (5, 63, 8)])
def test_the_kernel_writes_only_its_outputs_and_reads_only_its_inputs(dev, rows, N, S):
    """framed buffers (tests/framed.py): NaN, +3e38 and -3e38 guards around the rows and in the padding of ld, every output in a frame of
    its own.  A read outside a row changes the kept set or wins the draw; a write outside an output changes a guard."""
    from viewformer_amd import _lib, ops
    x, kinds, rid = R.inputs(rows, N, shift=0)
    T, top_k, top_p, seed = 2.0, 64, 0.9, 5
    want = ops.sample_rows(x[:, :N].contiguous().to(dev), rows, N, temperature=T, top_k=top_k, top_p=top_p, seed=seed, row_id=rid.to(dev),
                           n_samples=S, want=OUT)
    fx = Frame(rows, N, N + R.PAD, torch.float32, dev).load(x[:, :N])
    fr = Frame(1, rows, rows, torch.int64, dev).load(rid)
    outs = dict(idx=Frame(rows, S, S, torch.int64, dev), logp=Frame(rows, S, S, torch.float32, dev),
                kept=Frame(1, rows, rows, torch.int32, dev), thr=Frame(1, rows, rows, torch.float32, dev))
    for fill in (None, 3e38, -3e38):
        if fill is not None:
            fx.refill(fill)
            for f in outs.values():
                f.ibits.fill_(f.sentinel)
        st = _lib.load().vf_sample_rows_f32(ctypes.c_void_p(fx.ptr), rows, N, N + R.PAD, T, top_k, top_p, seed, ctypes.c_void_p(fr.ptr), S,
                                            *(ctypes.c_void_p(outs[k].ptr) for k in OUT), _strm())
        assert st == 0
        torch.cuda.synchronize()
        for name, f in [('logits', fx), ('row_id', fr)] + list(outs.items()):
            assert f.violations() == [], (name, fill, f.violations())
        _same_bits({k: outs[k].logical().view(want[k].shape) for k in OUT}, want, f'framed, guards {fill}')


@pytest.mark.parametrize('L', [1, 63, 64, 65])
def test_the_log_likelihood_is_one_chain_in_token_order(dev, L):
    from viewformer_amd import _lib, ops
    for views, S in ((1, 1), (5, 3), (3, 8)):
        lp = (torch.from_numpy(R.rng(40 + L + S).standard_normal((views * L, S)).astype(np.float32)) * 3.0 - 4.0)
        got = ops.sample_views(lp.to(dev), views, L, S).cpu()
        want = torch.stack([R.in_order_sum(lp.view(views, L, S)[:, :, s]) for s in range(S)], 1)
        assert torch.equal(_bits(got), _bits(want)), (L, views, S)
    fl = Frame(views * L, S, S, torch.float32, dev).load(lp)
    fo = Frame(views, S, S, torch.float32, dev)
    assert _lib.load().vf_sample_views_f32(ctypes.c_void_p(fl.ptr), views, L, S, ctypes.c_void_p(fo.ptr), _strm()) == 0
    torch.cuda.synchronize()
    assert fl.violations() == [] and fo.violations() == []
    assert torch.equal(_bits(fo.logical().cpu()), _bits(want))


# ------------------------------------------------------------------ the model and the renderer
SMALL = dict(n_embeddings=128, n_head=2, d_model=128, n_layer=2, token_image_size=8, pose_multiplier=0.2)      # 8 x 8 tokens, head dim 64
SMALL_VQ = dict(ch=32, ch_mult=[1, 2, 4], num_res_blocks=1, attn_resolutions=[16], image_size=32, z_channels=32, embed_dim=32, n_embed=128)
B_, C_, N_, L_ = 2, 3, 8, 64
_models = {}


def _setup(dev, arm):
    """the tiny model of tests/test_hip_score.py: model, cache, poses and the parent route's logits, built once per arm, left unchanged"""
    from viewformer_amd import geometry
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    if arm not in _models:
        cfg = MIGTConfig(sequence_size=C_ + 1, n_loss_skip=1, localization_weight='1', **SMALL)
        sd = make_migt_weights(cfg, seed=1, std=0.05)
        m = MIGT(cfg, precision=arm).load_state_dict(sd).to(dev)
        ctx = torch.from_numpy(R.rng(77).integers(0, cfg.n_embeddings, size=(B_, C_, 8, 8))).to(torch.int32)
        _, cams = synthetic_scene_batch(B_, C_ + N_, 8, 78)
        cams = torch.from_numpy(cams)
        p = geometry.normalize_cameras(geometry.to_relative_cameras(cams)[0])
        cpos, qpos = p[:, :C_].contiguous(), p[:, C_:].contiguous()
        cache = m.prefill_context(ctx, cpos)
        lg = m.generate_from_context(cache, qpos, codes_only=False)
        _models[arm] = types.SimpleNamespace(cfg=cfg, sd=sd, m=m, ctx=ctx, cpos=cpos, qpos=qpos, cams=cams, cache=cache, lg=lg)
    return _models[arm]


def _promised_row_ids(B, N, L, view0=0):
    b = np.arange(B, dtype=np.int64).reshape(B, 1) << 32
    return (b + (np.arange(N * L, dtype=np.int64) + view0 * L).reshape(1, N * L)).reshape(-1)


def _rows_of(t, S):
    """[B,N,S,t,t] -> [B*N*L][S]"""
    return t.reshape(B_, -1, S, L_).permute(0, 1, 3, 2).reshape(-1, S)


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_sample_from_context_against_the_reference_sampler(dev, arm):
    s = _setup(dev, arm)
    nE = s.cfg.n_embeddings
    z = s.lg.view(-1, nE).cpu().numpy()
    rid = _promised_row_ids(B_, N_, L_)
    cases = exempt = 0
    for S, T, top_k, top_p, seed in ((3, 1.0, 0, 1.0, 0), (8, 0.5, 16, 0.9, 5), (1, 2.0, 0, 0.5, 9)):
        out = s.m.sample_from_context(s.cache, s.qpos, n_samples=S, temperature=T, top_k=top_k, top_p=top_p, seed=seed, return_logits=True)
        assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == dict(
            codes=((B_, N_, S, 8, 8), torch.int64), token_log_prob=((B_, N_, S, 8, 8), torch.float32), log_likelihood=((B_, N_, S), torch.float32),
            kept=((B_, N_, 8, 8), torch.int32), logits=((B_, N_, 8, 8, nE), torch.float32))
        assert torch.equal(_bits(out['logits']), _bits(s.lg))                         # the bits of generate_from_context(codes_only=False)
        ref = R.sample_ref(z, T, top_k, top_p, seed, rid, S)
        got = dict(idx=_rows_of(out['codes'], S), logp=_rows_of(out['token_log_prob'], S), kept=out['kept'].reshape(-1))
        j = R.judge(got, ref, top_p, *CONSTANTS)
        assert j['errors'] == [], j['errors']
        _note(f'model {arm}', j)
        cases, exempt = cases + j['cases'], exempt + j['exempt']
        # the log-likelihood is the in-order chain of the tokens' log-probabilities
        tlp = out['token_log_prob'].cpu().reshape(B_ * N_ * S, L_)
        assert torch.equal(_bits(out['log_likelihood'].cpu().reshape(-1)), _bits(R.in_order_sum(tlp)))
    assert exempt <= R.CAP * cases, f'{exempt} of {cases} cases exempt'
    # top_k = 1 is generate_from_context, whatever the seed (on the tokens with a unique maximum: nearly all)
    uniq = (s.lg == s.lg.max(-1, keepdim=True).values).sum(-1) == 1                   # [B,N,t,t]
    assert float(uniq.float().mean()) > 0.9
    gen = s.m.generate_from_context(s.cache, s.qpos)
    for seed in (0, 3):
        one = s.m.sample_from_context(s.cache, s.qpos, n_samples=2, top_k=1, seed=seed)
        u = uniq[:, :, None].expand(-1, -1, 2, -1, -1)
        assert torch.equal(one['codes'][u], gen[:, :, None].expand(-1, -1, 2, -1, -1)[u]) and bool((one['token_log_prob'][u] == 0).all())
        assert bool((one['kept'][uniq] == 1).all())
        if bool(uniq.all()):
            assert bool((one['log_likelihood'] == 0).all())
    # N = 0
    empty = s.m.sample_from_context(s.cache, s.qpos[:, :0], n_samples=3, return_logits=True)
    assert {k: tuple(v.shape) for k, v in empty.items()} == dict(codes=(B_, 0, 3, 8, 8), token_log_prob=(B_, 0, 3, 8, 8),
                                                                 log_likelihood=(B_, 0, 3), kept=(B_, 0, 8, 8), logits=(B_, 0, 8, 8, nE))
    assert empty['codes'].dtype == torch.int64 and empty['kept'].dtype == torch.int32


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_scoring_the_sampled_codes_gives_their_log_probability(dev, arm):
    """T = 1, no filters: the distribution drawn from is the model's, so score_from_context of a sampled view returns the sample's
    token_log_prob — within the model-level bound of the scoring tests: (c + 1) x 2^-24 x (|logit of the code| + magnitude of lse), c the
    row kernel's constant for lse there"""
    import score_kernels_ref as SC
    import test_hip_score as GS
    s = _setup(dev, arm)
    nE, S = s.cfg.n_embeddings, 2
    out = s.m.sample_from_context(s.cache, s.qpos, n_samples=S, seed=4)
    z = s.lg.view(-1, nE)
    for k in range(S):
        codes = out['codes'][:, :, k]
        sc = s.m.score_from_context(s.cache, s.qpos, codes)
        _, mag = SC.token_log_prob(z, codes.reshape(-1))
        r = SC.worst_ratio(sc['token_log_prob'].reshape(-1), out['token_log_prob'][:, :, k].reshape(-1).double(), mag)
        print(f'{arm} sample {k}: score vs sample token_log_prob worst {r:.3f} x 2^-24 x magnitude')
        assert r <= GS.C['rows lse'] + 1, r


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_renderer_sample_chunks_scenes_images_and_render_unchanged(dev, arm):
    from viewformer_amd import ops
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.render import ViewRenderer, query_poses, sample_views
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_vqgan_weights
    s = _setup(dev, arm)
    vcfg = VQGANConfig(**SMALL_VQ)
    vq = VQGAN(vcfg, data_format='NHWC').load_state_dict(make_vqgan_weights(vcfg, seed=1, codebook_scale=0.05)).to(dev)
    r = ViewRenderer(s.m, vq).set_context(codes=s.ctx, cameras=s.cams[:, :C_])
    q = s.cams[:, C_:].to(dev)
    before = r.render(q, return_codes=True)
    kw = dict(n_samples=3, temperature=0.8, top_k=32, top_p=0.9, seed=6, return_codes=True)
    one = r.sample(q, **kw)
    assert {k: tuple(v.shape) for k, v in one.items()} == dict(
        generated_images=(B_, N_, 3, 32, 32, 3), log_likelihood=(B_, N_, 3), generated_codes=(B_, N_, 3, 8, 8),
        token_log_prob=(B_, N_, 3, 8, 8), kept=(B_, N_, 8, 8))
    assert one['generated_images'].dtype == torch.uint8
    assert set(r.sample(q, n_samples=3)) == {'generated_images', 'log_likelihood'}
    # a view's result does not depend on the chunking
    for cap in (1, 3):
        for k, v in r.sample(q, max_views_per_call=cap, **kw).items():
            assert torch.equal(v, one[k]), (cap, k)
    # ... nor on the other scenes of the batch.  The noise is keyed by the scene's NUMBER in its batch: scene 0 alone is scene 0, bit for
    # bit; scene 1 alone is scene 0 of its own batch, so what does not depend on the noise is compared — the kept sets, and top_k = 1
    alone = ViewRenderer(s.m, vq).set_context(codes=s.ctx[:1], cameras=s.cams[:1, :C_]).sample(q[:1], **kw)
    for k, v in alone.items():
        assert torch.equal(v, one[k][:1]), k
    r1 = ViewRenderer(s.m, vq).set_context(codes=s.ctx[1:], cameras=s.cams[1:, :C_])
    assert torch.equal(r1.sample(q[1:], **kw)['kept'], one['kept'][1:])
    k1 = dict(n_samples=2, top_k=1, seed=6, return_codes=True)
    for k, v in r1.sample(q[1:], **k1).items():
        assert torch.equal(v, r.sample(q, **k1)[k][1:]), k
    # the renderer's poses are the model's
    direct = s.m.sample_from_context(r.cache, query_poses(q, r.transform), n_samples=3, temperature=0.8, top_k=32, top_p=0.9, seed=6)
    assert torch.equal(direct['codes'], one['generated_codes']) and torch.equal(direct['log_likelihood'], one['log_likelihood'])
    # the images are the decoder's output of the codes
    for b, n, k in ((0, 0, 0), (1, 7, 2), (0, 3, 1)):
        dec = vq.decode_code(one['generated_codes'][b, n, k][None]).contiguous()
        assert torch.equal(ops.postprocess_u8(dec)[0], one['generated_images'][b, n, k])
    # the one-call form
    for k, v in sample_views(s.m, vq, None, s.cams[:, :C_], q, codes=s.ctx, **kw).items():
        assert torch.equal(v, one[k]), k
    # top_k = 1 is render
    greedy = r.sample(q, n_samples=1, top_k=1, return_codes=True)
    assert torch.equal(greedy['generated_codes'][:, :, 0], before['generated_codes'])
    assert torch.equal(greedy['generated_images'][:, :, 0], before['generated_images'])
    # render is what it was
    after = r.render(q, return_codes=True)
    for k, v in before.items():
        assert torch.equal(_bits(v), _bits(after[k])), k
    assert torch.equal(r.render(q)['generated_images'], before['generated_images'])
    # N = 0
    empty = r.sample(q[:, :0], n_samples=2)
    assert tuple(empty['generated_images'].shape) == (B_, 0, 2, 32, 32, 3) and tuple(empty['log_likelihood'].shape) == (B_, 0, 2)


def test_sample_refusals(dev):
    from viewformer_amd import _lib
    from viewformer_amd.migt import MIGT
    s = _setup(dev, 'bf16')
    other = MIGT(s.cfg, precision='bf16').load_state_dict(s.sd).to(dev)
    with pytest.raises(ValueError):
        other.sample_from_context(s.cache, s.qpos)                                   # a foreign cache
    with pytest.raises(ValueError):
        _setup(dev, 'f32').m.sample_from_context(s.cache, s.qpos)                    # another arm's cache
    with pytest.raises(_lib.VfError):                                                # no fp8 arm of the prefix attention, and no fallback
        MIGT(s.cfg, precision='bf16', attention='fp8').load_state_dict(s.sd).to(dev).sample_from_context(s.cache, s.qpos)
    with pytest.raises(TypeError):
        s.m.sample_from_context(None, s.qpos)
    with pytest.raises(ValueError):
        s.m.sample_from_context(s.cache, s.qpos[:1])                                 # another batch size
    with pytest.raises(ValueError):
        s.m.sample_from_context(s.cache, s.qpos[..., :6])
    for bad in (dict(n_samples=0), dict(n_samples=65536), dict(temperature=0.0), dict(temperature=float('inf')), dict(top_p=0.0),
                dict(top_p=float('nan')), dict(top_k=-1), dict(view0=-1), dict(view0=1 << 26)):
        with pytest.raises(ValueError):
            s.m.sample_from_context(s.cache, s.qpos, **bad)
    with pytest.raises(_lib.VfError):                                                # the kernel's own refusals reach the caller
        from viewformer_amd import ops
        ops.sample_rows(torch.zeros((2, 8), device=dev), 2, 8, temperature=-1.0)
