"""GPU: scoring photos at candidate cameras (csrc/lmhead_score.hip, MIGT.score_from_context, ViewRenderer.score) — the fused LM-head
kernel and the row kernel one by one against the float64 references of tests/score_kernels_ref.py (pinned on the CPU by
tests/test_score_ref_host.py), then the model and the renderer.

Exact class (idx, max_logit, target_logit: selections): ``torch.equal`` to what the existing kernels give — ops.lmhead_argmax_bf16 and
the gather from vf_gemm_bf16's logits.  Rounded class (lse, entropy): |got - want| <= c x 2^-24 x magnitude, the float64 reference
computed FROM vf_gemm_bf16's logits (an existing kernel with the same accumulation: the comparison isolates the new epilogue).  ``TABLE``
holds one (basis, c) per kernel and statistic: basis = the worst error of the float32 CPU restatement of the kernel's formula against
float64 on these very inputs, as the host file measures and prints it, c = 4 x basis rounded up to a power of two — never a figure taken
from the kernel.  Every measured worst ratio goes to the parity report (profiles/score_kernels_parity.txt)."""
import ctypes
import itertools
import math
import types

import numpy as np
import pytest
import torch

import score_kernels_ref as S
from conftest import parity_report
from framed import Frame

pytestmark = pytest.mark.gpu

# kernel statistic: (basis, c), see the module docstring; test_score_ref_host.py::test_the_gpu_tests_constants_are_calibrated_on_its_inputs
TABLE = {
    'fused lse': (0.91, 4.0),
    'fused entropy': (0.82, 4.0),
    'rows lse': (1.33, 8.0),
    'rows entropy': (1.17, 8.0),
}
C = {k: c for k, (b, c) in TABLE.items()}
_worst, _c_used = {}, {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        parity_report(test='score_kernels', kernel=k, worst_ratio=_worst[k], c=_c_used.get(k, 0.0), basis=TABLE.get(k, (0.0, 0.0))[0],
                      unit='2^-24 x magnitude' if k in _c_used else 'mismatching elements')


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _exact(name, got, want, what=''):
    ok = got.dtype == want.dtype and torch.equal(got, want)
    _worst[name] = max(_worst.get(name, 0), 0 if ok else int((got != want).sum()) or 1)
    assert ok, f'{name} {what}: differs from the existing kernel'


def _close(name, got, want, mag, what='', c=None):
    c = C[name] if c is None else c
    _c_used[name] = c
    r = S.worst_ratio(got.to(want.device), want, mag)
    _worst[name] = max(_worst.get(name, 0.0), r)
    print(f'{name} {what}: worst {r:.3f} x 2^-24 x magnitude (c = {c:g})')
    assert r <= c, f'{name} {what}: {r:.3f} x 2^-24 x magnitude exceeds c = {c:g}'


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f'{what}: {k} differs in its bits'


def _gemm_logits(h, wp, M, K, N):
    from viewformer_amd import ops
    out = torch.empty((M, N), dtype=torch.float32, device=h.device)
    ops.igemm(h.contiguous(), wp, M, K, N, out, bf16=True, a16=h.dtype == torch.bfloat16)
    return out


# ------------------------------------------------------------------ the fused kernel
_fused_cache = {}


def _fused_case(dev, M, K, N, h16):
    """inputs on the device, vf_gemm_bf16's logits and their float64 statistics: computed once per case, shared, left unchanged"""
    from viewformer_amd import ops
    key = (M, K, N, h16)
    if key not in _fused_cache:
        h, wte, tgt, kinds = S.fused_inputs(M, K, N)
        h = h.to(dev).to(torch.bfloat16 if h16 else torch.float32)
        wp = ops.pack_dense_nk_bf16(wte.to(dev), n_rows=N)
        tgt = tgt.to(dev)
        z = _gemm_logits(h, wp, M, K, N)
        _fused_cache[key] = (h, wp, tgt, kinds, z, S.score_stats(z, tgt))
    return _fused_cache[key]


@pytest.mark.parametrize('h16', [False, True])
@pytest.mark.parametrize('K,N', S.FUSED_KN)
@pytest.mark.parametrize('M', S.FUSED_M)
def test_fused_head_statistics(dev, M, K, N, h16):
    """rows of every kind of S.fused_inputs (spread +-60, the maximum in the first tile / in the last tile of the last wave, exact ties
    across lanes, waves and tiles, a nearly uniform row), targets at 0, 31, 32, N/4 - 1, N/4, N - 1, -1 and N; compact and padded ldh"""
    from viewformer_amd import ops
    h, wp, tgt, kinds, z, ref = _fused_case(dev, M, K, N, h16)
    am, amx = ops.lmhead_argmax_bf16(h, wp, M, K, N, want_max=True)
    hp = torch.zeros((M, K + S.LDH_PAD), dtype=h.dtype, device=dev)
    hp[:, :K] = h
    for what, hh in (('compact', h), ('padded ldh', hp[:, :K])):
        got = ops.lmhead_score_bf16(hh, wp, M, K, N, target=tgt)
        what = f'M {M} K {K} N {N} h16 {h16} {what}'
        _exact('fused idx', got['idx'], am, what)
        _exact('fused max_logit', got['max_logit'], amx, what)
        _exact('fused target_logit', got['target_logit'], ref['target_logit'][0].float(), what)
        _close('fused lse', got['lse'], *ref['lse'], what)
        _close('fused entropy', got['entropy'], *ref['entropy'], what)
    assert bool(torch.isinf(got['target_logit'][tgt < 0]).all()) and bool(torch.isinf(got['target_logit'][tgt >= N]).all())
    # the existing arg-max is the arg-max of those logits, ties to the lowest index (what makes the comparison above the issue's)
    assert torch.equal(am, ref['idx'][0]) and torch.equal(amx, ref['max_logit'][0].float())


def test_fused_head_every_combination_of_outputs_and_a_row_alone(dev):
    """a row's five outputs are bit-identical whichever outputs are requested, and whether the row is launched alone or among others"""
    from viewformer_amd import ops
    M, K, N = 65, 128, 1024
    h, wp, tgt, _, _, _ = _fused_case(dev, M, K, N, False)
    full = ops.lmhead_score_bf16(h, wp, M, K, N, target=tgt)
    for n in range(1, 5):
        for want in itertools.combinations(S.OUTPUTS, n):
            got = ops.lmhead_score_bf16(h, wp, M, K, N, target=tgt if 'target_logit' in want else None, want=want)
            assert tuple(got) == want
            _same_bits(got, {k: full[k] for k in want}, f'want {want}')
    for K2, N2 in S.FUSED_KN:
        h, wp, tgt, _, _, _ = _fused_case(dev, M, K2, N2, False)
        among = ops.lmhead_score_bf16(h, wp, M, K2, N2, target=tgt)
        alone = ops.lmhead_score_bf16(h[40:41], wp, 1, K2, N2, target=tgt[40:41].contiguous())
        _same_bits(alone, {k: v[40:41] for k, v in among.items()}, f'row 40 alone, K {K2} N {N2}')
        head = ops.lmhead_score_bf16(h[:33], wp, 33, K2, N2, target=tgt[:33].contiguous())
        _same_bits(head, {k: v[:33] for k, v in among.items()}, f'rows 0..32 alone, K {K2} N {N2}')


@pytest.mark.parametrize('h16', [False, True])
@pytest.mark.parametrize('M,K,N', [(33, 128, 128), (65, 768, 1024)])
def test_fused_head_writes_only_its_outputs_and_reads_only_its_inputs(dev, M, K, N, h16):
    """framed buffers (tests/framed.py): NaN guards around h's rows (and in the padding of ldh), the packing and the targets; every output
    in a frame of its own.  A read outside an input reaches lse as a NaN; a write outside an output changes a guard."""
    from viewformer_amd import _lib, ops
    h, wp, tgt, _, _, _ = _fused_case(dev, M, K, N, h16)
    want = ops.lmhead_score_bf16(h, wp, M, K, N, target=tgt)
    fh = Frame(M, K, K + S.LDH_PAD, h.dtype, dev).load(h)
    fw = Frame.raw(wp.numel() * 2, dev, dtype=torch.bfloat16).load(wp)
    ft = Frame(1, M, M, torch.int32, dev).load(tgt)
    outs = {k: Frame(1, M, M, torch.int64 if k == 'idx' else torch.float32, dev) for k in S.OUTPUTS}
    for fill in (None, 3e38, -3e38):
        if fill is not None:
            fh.refill(fill)
            for f in outs.values():
                f.ibits.fill_(f.sentinel)
        st = _lib.load().vf_lmhead_score_bf16(ctypes.c_void_p(fh.ptr), 1 if h16 else 0, K + S.LDH_PAD, ctypes.c_void_p(fw.ptr), M, K, N,
                                              ctypes.c_void_p(ft.ptr), *(ctypes.c_void_p(outs[k].ptr) for k in S.OUTPUTS), _strm())
        assert st == 0
        torch.cuda.synchronize()
        for name, f in [('h', fh), ('w_packed', fw), ('target', ft)] + list(outs.items()):
            assert f.violations() == [], (name, fill, f.violations())
        _same_bits({k: outs[k].logical().view(-1) for k in S.OUTPUTS}, want, f'framed, guards {fill}')


# ------------------------------------------------------------------ the row kernel
@pytest.mark.parametrize('N', S.ROWS_N)
def test_row_kernel_statistics(dev, N):
    """ld = N + 4 with +3e38 in the pad (a read past N wins the row); -inf codes; a row of nothing but -inf gives idx 0, max = lse = -inf
    and a NaN entropy — NaN and -inf exactly where the float64 reference has them"""
    from viewformer_amd import ops
    for rows in (1, 5):
        for kind in S.ROWS_KINDS:
            x, tgt = S.rows_inputs(rows, N, kind)
            ref = S.score_stats(x[:, :N], tgt)
            got = ops.logits_score(x.to(dev), rows, N, target=tgt.to(dev), ld=N + S.ROWS_PAD)
            what = f'N {N} rows {rows} {kind}'
            for k in ('idx', 'max_logit', 'target_logit'):
                bad = S.mismatches(got[k].cpu(), ref[k][0])
                _worst[f'rows {k}'] = max(_worst.get(f'rows {k}', 0), bad)
                assert bad == 0, f'rows {k} {what}: {bad} elements differ from the reference'
            assert got['idx'].dtype == torch.int64
            for k in ('lse', 'entropy'):
                g = got[k].cpu()
                bad, fin = S.split_special(g, ref[k][0])
                assert bad == 0, f'rows {k} {what}: NaN / inf not where the reference has them'
                if bool(fin.any()):
                    _close(f'rows {k}', g[fin], ref[k][0][fin], ref[k][1][fin], what)
    # compact rows, and every combination of outputs gives the same bits
    x, tgt = S.rows_inputs(5, N, 'normal')
    xc = x[:, :N].contiguous().to(dev)
    full = ops.logits_score(xc, 5, N, target=tgt.to(dev))
    _same_bits(full, ops.logits_score(x.to(dev), 5, N, target=tgt.to(dev), ld=N + S.ROWS_PAD), f'N {N} compact')
    for n in range(1, 5):
        for want in itertools.combinations(S.OUTPUTS, n):
            got = ops.logits_score(xc, 5, N, target=tgt.to(dev) if 'target_logit' in want else None, want=want)
            _same_bits(got, {k: full[k] for k in want}, f'N {N} want {want}')


def test_row_kernel_in_frames_and_the_view_summary(dev):
    from viewformer_amd import _lib, ops
    rows, N = 7, 1026
    x, tgt = S.rows_inputs(rows, N, 'spread')
    want = ops.logits_score(x[:, :N].contiguous().to(dev), rows, N, target=tgt.to(dev))
    fx = Frame(rows, N, N + S.ROWS_PAD, torch.float32, dev).load(x[:, :N])
    ft = Frame(1, rows, rows, torch.int32, dev).load(tgt)
    outs = {k: Frame(1, rows, rows, torch.int64 if k == 'idx' else torch.float32, dev) for k in S.OUTPUTS}
    for fill in (None, 3e38):
        if fill is not None:
            fx.refill(fill)
            for f in outs.values():
                f.ibits.fill_(f.sentinel)
        st = _lib.load().vf_logits_score_f32(ctypes.c_void_p(fx.ptr), rows, N, N + S.ROWS_PAD, ctypes.c_void_p(ft.ptr),
                                             *(ctypes.c_void_p(outs[k].ptr) for k in S.OUTPUTS), _strm())
        assert st == 0
        torch.cuda.synchronize()
        for name, f in [('logits', fx), ('target', ft)] + list(outs.items()):
            assert f.violations() == [], (name, fill, f.violations())
        _same_bits({k: outs[k].logical().view(-1) for k in S.OUTPUTS}, want, f'framed rows, guards {fill}')
    # the per-view summary: the same float32 statements on the CPU, bit for bit; the sum in token order
    views, L = 3, 64
    x, tgt = S.rows_inputs(views * L, 65, 'normal')
    tgt[::3] = torch.from_numpy(S.rows_score_f32(x[:, :65].numpy())['idx'][::3]).to(torch.int32)       # some hits
    st = ops.logits_score(x.to(dev), views * L, 65, target=tgt.to(dev), ld=65 + S.ROWS_PAD)
    tlp, conf, ll, acc = (t.cpu() for t in ops.score_views(st, tgt.to(dev), views, L))
    c = {k: v.cpu() for k, v in st.items()}
    assert torch.equal(tlp, c['target_logit'] - c['lse']) and torch.equal(conf, c['max_logit'] - c['lse'])
    assert torch.equal(ll, _in_order_sum(tlp.view(views, L)))
    assert torch.equal(acc, (c['idx'] == tgt.long()).view(views, L).float().sum(1) / L)


def _in_order_sum(x):
    s = x[:, 0].clone()
    for l in range(1, x.shape[1]):
        s = s + x[:, l]
    return s


# ------------------------------------------------------------------ the model and the renderer
SMALL = dict(n_embeddings=128, n_head=2, d_model=128, n_layer=2, token_image_size=8, pose_multiplier=0.2)      # 8 x 8 tokens, head dim 64
SMALL_VQ = dict(ch=32, ch_mult=[1, 2, 4], num_res_blocks=1, attn_resolutions=[16], image_size=32, z_channels=32, embed_dim=32, n_embed=128)
B_, C_, N_ = 2, 3, 8
_models = {}


def _poses(B, C, N, seed):
    from viewformer_amd import geometry
    from viewformer_amd.weights import synthetic_scene_batch
    _, cams = synthetic_scene_batch(B, C + N, 8, seed)
    p = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0])
    return p[:, :C].contiguous(), p[:, C:].contiguous(), torch.from_numpy(cams)


def _setup(dev, arm, size='small'):
    """model, cache, poses, photo codes and the parent route's logits for them: built once per (arm, size), shared, left unchanged"""
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    key = (arm, size)
    if key not in _models:
        kw = SMALL if size == 'small' else dict(n_layer=2, pose_multiplier=0.2)
        cfg = MIGTConfig(sequence_size=C_ + 1, n_loss_skip=1, localization_weight='1', **kw)
        sd = make_migt_weights(cfg, seed=1, std=0.05 if size == 'small' else 0.03)
        m = MIGT(cfg, precision=arm).load_state_dict(sd).to(dev)
        g = S.rng(77)
        ctx = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(B_, C_, 8, 8))).to(torch.int32)
        photos = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(B_, N_, 8, 8))).to(torch.int32)
        cpos, qpos, cams = _poses(B_, C_, N_, 78)
        cache = m.prefill_context(ctx, cpos)
        lg = m.generate_from_context(cache, qpos, codes_only=False)
        _models[key] = types.SimpleNamespace(cfg=cfg, sd=sd, m=m, ctx=ctx, photos=photos.to(dev), cpos=cpos, qpos=qpos, cams=cams, cache=cache, lg=lg)
    return _models[key]


@pytest.mark.parametrize('arm,size,fused', [('bf16', 'small', True), ('bf16', 'small', False), ('f32', 'small', False),
                                            ('bf16', 'full_width', True), ('bf16', 'full_width', False)])
def test_score_from_context_against_the_parent_route(dev, arm, size, fused):
    """predicted_codes == generate_from_context(codes_only=True); token_log_prob against log_softmax of the parent route's logits gathered
    at the codes, float64, at the kernel's tolerance: the target's logit is exact, lse is within c units of its magnitude and the
    subtraction rounds once more, so (c + 1) x 2^-24 x (|target logit| + magnitude of lse).  Confidence and entropy likewise."""
    s = _setup(dev, arm, size)
    nE = s.cfg.n_embeddings
    out = s.m.score_from_context(s.cache, s.qpos, s.photos, fused=fused)
    if not fused:                                                                    # the default route
        for k, v in s.m.score_from_context(s.cache, s.qpos, s.photos).items():
            assert torch.equal(_bits(v), _bits(out[k])), k
    assert {k: tuple(v.shape) for k, v in out.items()} == dict(
        token_log_prob=(B_, N_, 8, 8), log_likelihood=(B_, N_), predicted_codes=(B_, N_, 8, 8), confidence=(B_, N_, 8, 8),
        entropy=(B_, N_, 8, 8), accuracy=(B_, N_))
    assert torch.equal(out['predicted_codes'], s.m.generate_from_context(s.cache, s.qpos, codes_only=True))
    z = s.lg.view(-1, nE)
    tgt = s.photos.reshape(-1)
    ref = S.score_stats(z, tgt)
    kern = 'fused' if fused else 'rows'
    c = C[f'{kern} lse']
    arm = f'{arm} {kern}'
    want, mag = S.token_log_prob(z, tgt)
    _close(f'model {arm} {size} token_log_prob', out['token_log_prob'].reshape(-1), want, mag, c=c + 1)
    _close(f'model {arm} {size} confidence', out['confidence'].reshape(-1), ref['max_logit'][0] - ref['lse'][0],
           ref['max_logit'][0].abs() + ref['lse'][1], c=c + 1)
    _close(f'model {arm} {size} entropy', out['entropy'].reshape(-1), *ref['entropy'], c=C[f'{kern} entropy'])
    assert torch.equal(out['log_likelihood'].cpu(), _in_order_sum(out['token_log_prob'].cpu().view(B_ * N_, 64)).view(B_, N_))
    assert torch.equal(out['accuracy'], (out['predicted_codes'] == s.photos).float().view(B_, N_, 64).sum(-1) / 64)
    # N = 0
    empty = s.m.score_from_context(s.cache, s.qpos[:, :0], s.photos[:, :0])
    assert tuple(empty['token_log_prob'].shape) == (B_, 0, 8, 8) and tuple(empty['log_likelihood'].shape) == (B_, 0)
    assert empty['predicted_codes'].dtype == torch.int64


@pytest.mark.parametrize('arm,fused', [('bf16', True), ('bf16', False), ('f32', False)])
def test_score_against_the_fp64_oracle_is_no_worse_than_the_parent_route(dev, arm, fused):
    """scene 0, cameras 0 and 1: the oracle's full pass [ctx, MASK] in float64 -> log_softmax at the photo's codes.  e_full: the parent
    route (generate_from_context(codes_only=False) + log_softmax + gather, float32 on the device); e_score: score_from_context."""
    from oracle import migt_oracle as mg
    s = _setup(dev, arm)
    nE = s.cfg.n_embeddings
    ids = torch.cat([s.ctx, torch.full_like(s.ctx[:, :1], nE)], 1).long()
    ref = torch.stack([mg.migt_forward(s.sd, s.cfg, ids[:1], torch.cat([s.cpos[:1], s.qpos[:1, n:n + 1]], 1), dtype=torch.float64)['logits'][0, -1]
                       for n in (0, 1)]).reshape(2 * 64, nE)
    tgt = s.photos[0, :2].reshape(-1).long().cpu()
    want = torch.log_softmax(ref, -1).gather(1, tgt[:, None])[:, 0]
    parent = torch.log_softmax(s.lg[0, :2].reshape(-1, nE), -1).gather(1, tgt.to(dev)[:, None])[:, 0].cpu().double()
    got = s.m.score_from_context(s.cache, s.qpos, s.photos, fused=fused)['token_log_prob'][0, :2].reshape(-1).cpu().double()
    e_full, e_score = float((parent - want).abs().max()), float((got - want).abs().max())
    parity_report(test='score_against_fp64_oracle', arm=arm, fused=fused, e_full=e_full, e_score=e_score, peak_log_prob=float(want.abs().max()))
    assert e_score <= 1.5 * e_full, (e_score, e_full)


@pytest.mark.parametrize('arm,fused', [('bf16', True), ('bf16', False), ('f32', False)])
def test_scoring_the_models_own_codes(dev, arm, fused):
    s = _setup(dev, arm)
    gen = s.m.generate_from_context(s.cache, s.qpos, codes_only=True)
    out = s.m.score_from_context(s.cache, s.qpos, gen, fused=fused)
    assert bool((out['accuracy'] == 1).all())
    assert torch.equal(out['token_log_prob'].view(torch.int32), out['confidence'].view(torch.int32))
    assert torch.equal(out['log_likelihood'].cpu(), _in_order_sum(out['token_log_prob'].cpu().view(B_ * N_, 64)).view(B_, N_))
    assert torch.equal(out['predicted_codes'], gen)
    # generate_from_context(return_confidence=True): the same launch's codes, confidence and entropy
    g2, conf, ent = s.m.generate_from_context(s.cache, s.qpos, codes_only=True, return_confidence=True)
    assert torch.equal(g2, gen)
    if not fused:                                                                    # (return_confidence takes the default route)
        assert torch.equal(conf.view(torch.int32), out['confidence'].view(torch.int32))
        assert torch.equal(ent.view(torch.int32), out['entropy'].view(torch.int32))


@pytest.mark.parametrize('size', ['small', 'full_width'])
def test_fused_and_unfused_routes_agree_on_the_bf16_arm(dev, size):
    """idx and the target's logit equal; lse and entropy: each route is within its c units of the float64 value of the same logits, so
    the two differ by at most c_fused + c_rows units (<= 2 c for the larger of the two)"""
    s = _setup(dev, 'bf16', size)
    nE, M = s.cfg.n_embeddings, B_ * N_ * 64
    tgt = s.photos.reshape(-1).contiguous()
    hf = s.m._query_rows(s.cache, torch.full((M,), s.m.mask_token, dtype=torch.int32, device=dev),
                         s.m._pose_embed(s.qpos.to(dev)).contiguous().view(B_ * N_, s.cfg.d_model), N_)
    a, b = s.m._lm_score(hf, M, tgt, fused=True), s.m._lm_score(hf, M, tgt, fused=False)
    assert torch.equal(a['idx'], b['idx']) and torch.equal(a['target_logit'], b['target_logit']) and torch.equal(a['max_logit'], b['max_logit'])
    ref = S.score_stats(s.lg.view(-1, nE), tgt)
    for k in ('lse', 'entropy'):
        _close(f'fused vs rows {k} {size}', a[k], b[k].double(), ref[k][1], c=C[f'fused {k}'] + C[f'rows {k}'])
    fa, fb = s.m.score_from_context(s.cache, s.qpos, s.photos, fused=True), s.m.score_from_context(s.cache, s.qpos, s.photos, fused=False)
    assert torch.equal(fa['predicted_codes'], fb['predicted_codes']) and torch.equal(fa['accuracy'], fb['accuracy'])


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_renderer_score_broadcast_chunks_and_confidence(dev, arm):
    """one photo broadcast over 8 cameras == the photo repeated 8 times; chunks of 4 + 4 views == one pass of 8; render with
    return_confidence generates the same images"""
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.render import ViewRenderer, query_poses, score_views
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_vqgan_weights
    s = _setup(dev, arm)
    vcfg = VQGANConfig(**SMALL_VQ)
    vq = VQGAN(vcfg, data_format='NHWC').load_state_dict(make_vqgan_weights(vcfg, seed=1, codebook_scale=0.05)).to(dev)
    r = ViewRenderer(s.m, vq).set_context(codes=s.ctx, cameras=s.cams[:, :C_])
    q = s.cams[:, C_:].to(dev)
    one = r.score(q, codes=s.photos)
    for k, v in r.score(q, codes=s.photos, max_views_per_call=4).items():
        assert torch.equal(v, one[k]), k
    single = r.score(q, codes=s.photos[:, :1])
    for k, v in r.score(q, codes=s.photos[:, :1].expand(B_, N_, 8, 8).contiguous()).items():
        assert torch.equal(v, single[k]), k
    assert torch.equal(single['predicted_codes'], one['predicted_codes'])            # the prediction does not depend on the photo
    assert torch.equal(single['token_log_prob'][:, 0], one['token_log_prob'][:, 0])
    # the renderer's poses are the model's: score() equals score_from_context at query_poses
    direct = s.m.score_from_context(r.cache, query_poses(q, r.transform), s.photos)
    for k in one:
        assert torch.equal(one[k], direct[k]), k
    # images in: encoded once, the same result as their codes; and the one-call form
    from viewformer_amd.weights import synthetic_scene_batch
    frames, _ = synthetic_scene_batch(B_, N_, 32, seed=79)
    frames = torch.from_numpy(frames).to(dev)
    codes = vq.encode(frames.view(-1, 32, 32, 3))[-1].view(B_, N_, 8, 8)
    by_img = r.score(q, images=frames)
    for k, v in r.score(q, codes=codes).items():
        assert torch.equal(v, by_img[k]), k
    for k, v in score_views(s.m, vq, None, s.cams[:, :C_], q, photos=frames, codes=s.ctx).items():
        assert torch.equal(v, by_img[k]), k
    # render
    plain, conf = r.render(q), r.render(q, return_confidence=True)
    assert torch.equal(plain['generated_images'], conf['generated_images'])
    assert tuple(conf['confidence'].shape) == (B_, N_, 8, 8) and tuple(conf['entropy'].shape) == (B_, N_, 8, 8)
    assert torch.equal(conf['confidence'], one['confidence']) and torch.equal(conf['entropy'], one['entropy'])
    assert bool((conf['confidence'] <= 0).all()) and bool((conf['entropy'] >= 0).all())
    both = r.render(q, return_codes=True, return_confidence=True)
    assert torch.equal(both['generated_images'], plain['generated_images']) and torch.equal(both['generated_codes'], one['predicted_codes'])


def test_score_refusals(dev):
    from viewformer_amd import _lib
    from viewformer_amd.migt import MIGT
    s = _setup(dev, 'bf16')
    other = MIGT(s.cfg, precision='bf16').load_state_dict(s.sd).to(dev)
    with pytest.raises(ValueError):
        other.score_from_context(s.cache, s.qpos, s.photos)                          # a foreign cache
    f32 = _setup(dev, 'f32')
    with pytest.raises(ValueError):
        f32.m.score_from_context(s.cache, s.qpos, s.photos)                          # another arm's cache
    with pytest.raises(_lib.VfError):                                                # no fp8 arm of the prefix attention, and no fallback
        MIGT(s.cfg, precision='bf16', attention='fp8').load_state_dict(s.sd).to(dev).score_from_context(s.cache, s.qpos, s.photos)
    with pytest.raises(TypeError):
        s.m.score_from_context(None, s.qpos, s.photos)
    with pytest.raises(ValueError):
        s.m.score_from_context(s.cache, s.qpos, s.photos.float())                    # float codes
    with pytest.raises(ValueError):
        s.m.score_from_context(s.cache, s.qpos, s.photos[:, :3])                     # 3 photos for 8 cameras
    with pytest.raises(ValueError):
        s.m.score_from_context(s.cache, s.qpos[:1], s.photos[:1])                    # another batch size
    with pytest.raises(ValueError):
        s.m.score_from_context(s.cache, s.qpos, s.photos.view(B_, N_, 64))           # another token shape
    with pytest.raises(ValueError):
        s.m.score_from_context(s.cache, s.qpos[..., :6], s.photos)
    with pytest.raises(ValueError):
        s.m.generate_from_context(s.cache, s.qpos, codes_only=False, return_confidence=True)
