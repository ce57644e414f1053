"""GPU: P photos against M cameras from M query views (csrc/match_views.hip, ops.match_views, MIGT.match_from_context,
ViewRenderer.match) — the kernel against the float32 restatement of tests/match_views_ref.py bit for bit (pinned on the CPU by
tests/test_match_views_ref_host.py), against the existing per-pair kernels, in framed buffers and for the independence of an element from
its launch; then the model and the renderer against the loop of ``score`` calls the feature replaces, element for element.

Exact class throughout: ``torch.equal`` on int32 views of the bits (match_views_ref.bits: every NaN counts as one pattern).  The distance
to the float64 reference, in units of the derived bound gamma_L x magnitude, is a sanity line for the parity report
(profiles/match_views_parity.txt), asserted <= 1 only because the restatement the bits are held to satisfies it on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import match_views_ref as R
from conftest import parity_report
from framed import Frame

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        parity_report(test='match_views', case=k, **_worst[k])


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(got, want, what):
    got = got.detach().cpu() if torch.is_tensor(got) else got
    a, b = R.bits(got), R.bits(want.detach().cpu() if torch.is_tensor(want) else want)
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    assert torch.equal(a, b), f'{what}: {int((a != b).sum())} of {a.numel()} elements differ in their bits'


def _same_any(got, want, what):
    """float32: the bits; anything else: dtype and values"""
    if got.dtype == torch.float32:
        return _same(got, want, what)
    assert got.dtype == want.dtype and torch.equal(got, want), what


_cases = {}


def _case(dev, c):
    """inputs on the host and on the device (the codes with the case's scene stride), the float64 reference and the float32 restatement:
    computed once per case, shared, left unchanged"""
    k = R.case_id(c)
    if k not in _cases:
        inp = R.inputs(c)
        B, P, L = c['B'], c['P'], c['L']
        codes = torch.from_numpy(inp['codes'])
        if c['stride'] == 'gap':                                                       # scenes P L + 3 apart, out-of-range codes between them
            buf = torch.full((B, P * L + 3), R.I32_MAX, dtype=torch.int32, device=dev)
            buf[:, :P * L] = codes.view(B, P * L).to(dev)
            dcodes = buf[:, :P * L].view(B, P, L)
            assert dcodes.stride() == (P * L + 3, L, 1)
        else:
            dcodes = codes.to(dev)
        d = dict(logits=torch.from_numpy(inp['logits']).to(dev), lse=torch.from_numpy(inp['lse']).to(dev),
                 idx=torch.from_numpy(inp['idx']).to(dev), codes=dcodes)
        _cases[k] = (inp, d, R.reference(inp, c), R.restated_f32(inp, c))
    return _cases[k]


def _run(d, c, **kw):
    from viewformer_amd import ops
    return ops.match_views(d['logits'], d['lse'], d['idx'], d['codes'], c['B'], c['M'], c['P'], c['L'], c['V'], ld=c['V'] + c['pad'], **kw)


# ------------------------------------------------------------------ a. the kernel, exact class
@pytest.mark.parametrize('c', R.CASES, ids=R.case_id)
def test_kernel_equals_the_float32_restatement_bit_for_bit(dev, c):
    inp, d, (ll64, mag, acc64), (ll32, acc32) = _case(dev, c)
    ll, acc = _run(d, c)
    assert tuple(ll.shape) == (c['B'], c['M'], c['P']) and ll.dtype == torch.float32 and ll.is_contiguous()
    r = R.worst_ratio(ll.cpu().numpy(), ll64, mag, c['L'])
    bad = int((R.bits(ll.cpu()) != R.bits(ll32)).sum()) + int((R.bits(acc.cpu()) != R.bits(acc32)).sum())
    _worst[R.case_id(c)] = dict(differing_elements=bad, worst_ratio_to_fp64=r, unit='gamma_L x magnitude', elements=ll.numel())
    print(f'{R.case_id(c)}: {bad} elements differ from the restatement; worst {r:.4f} x gamma_L x magnitude against float64')
    _same(ll, ll32, 'log_likelihood')
    _same(acc, acc32, 'accuracy')
    assert r <= 1.0


# ------------------------------------------------------------------ b. against the existing kernels, pair by pair
@pytest.mark.parametrize('c', [R.CASES[1], R.CASES[2]], ids=R.case_id)
def test_kernel_equals_score_views_of_logits_score_for_every_pair(dev, c):
    """photo p's codes as the target of every camera's rows: vf_logits_score_f32 gathers the target's logit, vf_score_views_f32 sums the
    view — the launches ``score_from_context`` makes for that photo.  lse and idx are the test's inputs on both sides.  (The two agree
    wherever lse is finite or the code lies in [0, V): the cases keep their out-of-range codes off the -inf row's token.)"""
    from viewformer_amd import ops
    inp, d, _, _ = _case(dev, c)
    B, M, P, L, V = c['B'], c['M'], c['P'], c['L'], c['V']
    t_inf, b_inf = inp['inf_row'] % L, inp['inf_row'] // (M * L)
    at_inf = inp['codes'][b_inf if inp['codes'].shape[0] > 1 else 0][:, t_inf]
    assert ((at_inf >= 0) & (at_inf < V)).all()
    ll, acc = _run(d, c)
    mx = torch.zeros(B * M * L, dtype=torch.float32, device=dev)                        # feeds confidence only
    for p in range(P):
        cp = d['codes'][:, p] if d['codes'].shape[0] == B else d['codes'][:, p].expand(B, L)
        target = cp[:, None, :].expand(B, M, L).reshape(-1).contiguous()
        tl = ops.logits_score(d['logits'], B * M * L, V, target=target, want=('target_logit',), ld=V + c['pad'])['target_logit']
        _, _, want_ll, want_acc = ops.score_views(dict(target_logit=tl, lse=d['lse'], max_logit=mx, idx=d['idx']), target, B * M, L)
        _same(ll[:, :, p], want_ll.view(B, M), f'log_likelihood of photo {p}')
        _same(acc[:, :, p], want_acc.view(B, M), f'accuracy of photo {p}')


# ------------------------------------------------------------------ c. footprint
def test_kernel_writes_only_its_outputs_and_reads_only_its_inputs(dev):
    """framed buffers (tests/framed.py): NaN guards around the logits and in the 5 columns between V and ld, around lse, idx and the codes
    and in the 3-int gap between the scenes' codes; both outputs in frames of their own.  Code -1 on the first row and code V on the
    last (and INT32_MAX there) would read the guards: nothing is read for them, their elements are -inf, not NaN."""
    from viewformer_amd import _lib
    c = dict(R.CASES[1])
    B, M, P, L, V = c['B'], c['M'], c['P'], c['L'], c['V']
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in R.inputs(c, seed=1).items()}
    first, last = (0, 0, 0), (B - 1, P - 1, L - 1)
    inp['codes'][first], inp['codes'][last], inp['codes'][B - 1, P - 2, L - 1] = -1, V, R.I32_MAX
    want_ll, want_acc = R.restated_f32(inp, c)
    rows, ld, stride = B * M * L, V + 5, P * L + 3
    fz = Frame(rows, V, ld, torch.float32, dev).load(torch.from_numpy(inp['logits'][:, :V]))
    fl = Frame(1, rows, rows, torch.float32, dev).load(torch.from_numpy(inp['lse']))
    fi = Frame(1, rows, rows, torch.int64, dev).load(torch.from_numpy(inp['idx']))
    fc = Frame(P, L, L, torch.int32, dev, batch=B, batch_stride=stride).load(torch.from_numpy(inp['codes']))
    outs = {k: Frame(B * M, P, P, torch.float32, dev) for k in ('log_likelihood', 'accuracy')}
    for fill in (None, 3e38):
        if fill is not None:
            fz.refill(fill)
            for f in outs.values():
                f.ibits.fill_(f.sentinel)
        st = _lib.load().vf_match_views_f32(ctypes.c_void_p(fz.ptr), ld, ctypes.c_void_p(fl.ptr), ctypes.c_void_p(fi.ptr), ctypes.c_void_p(fc.ptr),
                                            stride, B, M, P, L, V, ctypes.c_void_p(outs['log_likelihood'].ptr),
                                            ctypes.c_void_p(outs['accuracy'].ptr), _strm())
        assert st == 0
        torch.cuda.synchronize()
        for name, f in [('logits', fz), ('lse', fl), ('idx', fi), ('codes', fc)] + list(outs.items()):
            assert f.violations() == [], (name, fill, f.violations())
        ll = outs['log_likelihood'].logical().view(B, M, P)
        _same(ll, want_ll, f'framed log_likelihood, guards {fill}')
        _same(outs['accuracy'].logical().view(B, M, P), want_acc, f'framed accuracy, guards {fill}')
        # the -inf row lies in scene 1: the elements of scenes 0 and 2 next to the guards are -inf, not NaN and not 3e38
        assert inp['inf_row'] // (M * L) == 1
        assert bool(torch.isneginf(ll[0, :, 0]).all()) and bool(torch.isneginf(ll[B - 1, :, P - 1]).all()) and bool(torch.isneginf(ll[B - 1, :, P - 2]).all())


# ------------------------------------------------------------------ d. independence
@pytest.mark.parametrize('c', [R.CASES[3], R.CASES[5]], ids=R.case_id)
def test_an_elements_bits_do_not_depend_on_its_launch(dev, c):
    from viewformer_amd import ops
    inp, d, _, _ = _case(dev, c)
    B, M, P, L, V = c['B'], c['M'], c['P'], c['L'], c['V']
    ld = V + c['pad']
    ll, acc = _run(d, c)
    # without accuracy (and without idx)
    ll2, none = ops.match_views(d['logits'], d['lse'], None, d['codes'], B, M, P, L, V, ld=ld, want_accuracy=False)
    assert none is None
    _same(ll2, ll, 'log_likelihood without accuracy')
    # P split in two launches, at a photo that is no multiple of anything
    cut = 100
    for a, b in ((0, cut), (cut, P)):
        pl, pa = ops.match_views(d['logits'], d['lse'], d['idx'], d['codes'][:, a:b], B, M, b - a, L, V, ld=ld)
        _same(pl, ll[:, :, a:b], f'photos {a}..{b} alone: log_likelihood')
        _same(pa, acc[:, :, a:b], f'photos {a}..{b} alone: accuracy')
    # launched alone: B = M = P = 1, the first and the last element, one in the second workgroup's tile and one of the -inf row's view
    bm_inf = inp['inf_row'] // L
    for b, m, p in ((0, 0, 0), (B - 1, M - 1, P - 1), (B - 1, 0, 256), (bm_inf // M, bm_inf % M, 5)):
        r0 = (b * M + m) * L
        cb = d['codes'][b if d['codes'].shape[0] > 1 else 0, p].reshape(1, 1, L).contiguous()
        al, aa = ops.match_views(d['logits'][r0:r0 + L], d['lse'][r0:r0 + L].contiguous(), d['idx'][r0:r0 + L].contiguous(), cb, 1, 1, 1, L, V, ld=ld)
        _same(al.view(-1), ll[b, m, p].view(-1), f'element ({b}, {m}, {p}) alone: log_likelihood')
        _same(aa.view(-1), acc[b, m, p].view(-1), f'element ({b}, {m}, {p}) alone: accuracy')


# ------------------------------------------------------------------ e. the model
M_, P_ = 5, 7


def _setup(dev, arm):
    """the small model, cache, poses and photo codes of tests/test_hip_score.py (SMALL, B = 2, C = 3): built once per arm there, shared"""
    import test_hip_score as G
    return G._setup(dev, arm), G


def _against_score(m, cache, qpos, photos, out, what, n_context=None, shared=False):
    """for every (p, m): match[:, p, m] == score_from_context(one camera, one photo); the camera-only outputs == score_from_context's"""
    B = cache.B
    for p in range(photos.shape[1]):
        ph = photos[:, p:p + 1].expand(B, 1, *photos.shape[2:]) if shared else photos[:, p:p + 1]
        for k in range(qpos.shape[1]):
            kw = {} if n_context is None else dict(n_context=n_context[:, k:k + 1])
            one = m.score_from_context(cache, qpos[:, k:k + 1], ph, **kw)
            for key in ('log_likelihood', 'accuracy'):
                _same(out[key][:, p, k], one[key][:, 0], f'{what}: {key} of photo {p} at camera {k}')
    kw = {} if n_context is None else dict(n_context=n_context)
    ph = photos[:, :1].expand(B, 1, *photos.shape[2:]) if shared else photos[:, :1]
    cams = m.score_from_context(cache, qpos, ph, **kw)
    for key in ('predicted_codes', 'confidence', 'entropy'):
        _same_any(out[key], cams[key], f'{what}: {key}')


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_match_from_context_equals_score_from_context_pair_by_pair(dev, arm):
    """the feature's contract: P x M likelihoods from M query views, each the bits of the one-camera one-photo score"""
    (s, G) = _setup(dev, arm)
    B = G.B_
    qpos, photos = s.qpos[:, :M_].contiguous(), s.photos[:, :P_].contiguous()
    out = s.m.match_from_context(s.cache, qpos, photos)
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == dict(
        log_likelihood=((B, P_, M_), torch.float32), accuracy=((B, P_, M_), torch.float32), predicted_codes=((B, M_, 8, 8), torch.int64),
        confidence=((B, M_, 8, 8), torch.float32), entropy=((B, M_, 8, 8), torch.float32))
    assert bool(torch.isfinite(out['log_likelihood']).all())
    _against_score(s.m, s.cache, qpos, photos, out, f'{arm}')
    # a code outside the codebook: that photo's log-likelihood is -inf at every camera, the others keep their bits
    bad = photos.clone()
    bad[0, 2, 3, 4], bad[1, 6, 0, 0] = s.cfg.n_embeddings, -1
    ob = s.m.match_from_context(s.cache, qpos, bad)
    assert bool(torch.isneginf(ob['log_likelihood'][0, 2]).all()) and bool(torch.isneginf(ob['log_likelihood'][1, 6]).all())
    keep = torch.ones((B, P_), dtype=torch.bool, device=dev)
    keep[0, 2] = keep[1, 6] = False
    _same(ob['log_likelihood'][keep], out['log_likelihood'][keep], 'photos beside an out-of-range one')
    # int64 codes are taken as int32 ones are
    _same(s.m.match_from_context(s.cache, qpos, photos.long())['log_likelihood'], out['log_likelihood'], 'int64 codes')


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_match_from_context_with_context_lengths_and_a_shared_photo_set(dev, arm):
    (s, G) = _setup(dev, arm)
    qpos, photos = s.qpos[:, :M_].contiguous(), s.photos[:, :P_].contiguous()
    nc = torch.tensor([[3, 0, 2, 1, 3], [1, 2, 3, 0, 2]], dtype=torch.int32)           # per camera, in [0, C]
    out = s.m.match_from_context(s.cache, qpos, photos, n_context=nc)
    _against_score(s.m, s.cache, qpos, photos, out, f'{arm} n_context per camera', n_context=nc)
    full = s.m.match_from_context(s.cache, qpos, photos)
    assert not torch.equal(out['log_likelihood'], full['log_likelihood'])                # the lengths are not ignored
    shared = photos[1:2]                                                               # [1, P, t, t]: one photo set for both scenes
    out = s.m.match_from_context(s.cache, qpos, shared)
    assert tuple(out['log_likelihood'].shape) == (G.B_, P_, M_)
    _against_score(s.m, s.cache, qpos, shared, out, f'{arm} shared photo set', shared=True)
    _same(out['log_likelihood'][1], full['log_likelihood'][1], 'scene 1 with its own photos as the shared set')


@pytest.mark.parametrize('form', ['kv', 'e4m3'])
def test_match_from_context_on_packed_caches(dev, form):
    (s, G) = _setup(dev, 'bf16')
    qpos, photos = s.qpos[:, :M_].contiguous(), s.photos[:, :P_].contiguous()
    packed = s.cache.pack() if form == 'kv' else s.cache.pack('e4m3')
    out = s.m.match_from_context(packed, qpos, photos)
    _against_score(s.m, packed, qpos, photos, out, f'packed {form}')
    if form == 'kv':                                                                   # the K/V-only pack keeps every bit of the plain cache
        _same(out['log_likelihood'], s.m.match_from_context(s.cache, qpos, photos)['log_likelihood'], 'K/V-only pack against the plain cache')


def test_match_from_context_empty_and_refusals(dev):
    (s, G) = _setup(dev, 'bf16')
    B = G.B_
    qpos, photos = s.qpos[:, :M_].contiguous(), s.photos[:, :P_].contiguous()
    e = s.m.match_from_context(s.cache, qpos[:, :0], photos)
    assert tuple(e['log_likelihood'].shape) == (B, P_, 0) and tuple(e['accuracy'].shape) == (B, P_, 0)
    assert tuple(e['predicted_codes'].shape) == (B, 0, 8, 8) and e['predicted_codes'].dtype == torch.int64
    assert tuple(e['confidence'].shape) == (B, 0, 8, 8) and e['entropy'].dtype == torch.float32
    e = s.m.match_from_context(s.cache, qpos, photos[:, :0])
    assert tuple(e['log_likelihood'].shape) == (B, 0, M_) and e['log_likelihood'].dtype == torch.float32
    assert torch.equal(e['predicted_codes'], s.m.generate_from_context(s.cache, qpos, codes_only=True))
    with pytest.raises(TypeError):
        s.m.match_from_context(None, qpos, photos)
    for bad in (photos.float(), photos.bool(), photos.view(B, P_, 64), photos[:, :, :4], torch.cat([photos, photos[:1]], 0)):
        with pytest.raises(ValueError):
            s.m.match_from_context(s.cache, qpos, bad)
    for bad in (qpos[:1], qpos[..., :6]):
        with pytest.raises(ValueError):
            s.m.match_from_context(s.cache, bad, photos)
    with pytest.raises(ValueError):
        s.m.match_from_context(s.cache, qpos, photos, n_context=4)                     # C = 3


# ------------------------------------------------------------------ f. the renderer
def _first_argmax(x):
    return torch.from_numpy(np.argmax(x.cpu().numpy(), axis=-1))                         # numpy: the first maximum


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_renderer_match_equals_the_loop_of_score_calls(dev, arm):
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.render import ViewRenderer, match_views
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_vqgan_weights, synthetic_scene_batch
    (s, G) = _setup(dev, arm)
    B, C = G.B_, G.C_
    vcfg = VQGANConfig(**G.SMALL_VQ)
    vq = VQGAN(vcfg, data_format='NHWC').load_state_dict(make_vqgan_weights(vcfg, seed=1, codebook_scale=0.05)).to(dev)
    r = ViewRenderer(s.m, vq).set_context(codes=s.ctx, cameras=s.cams[:, :C])
    q = s.cams[:, C:C + M_].to(dev)
    photos = s.photos[:, :P_].contiguous()
    out = r.match(q, codes=photos)
    assert tuple(out['log_likelihood'].shape) == (B, P_, M_) and tuple(out['best_camera'].shape) == (B, P_) and tuple(out['best_photo'].shape) == (B, M_)
    assert out['best_camera'].dtype == torch.int64 and out['best_photo'].dtype == torch.int64
    for p in range(P_):                                                                # the loop the feature replaces: one photo against M cameras
        one = r.score(q, codes=photos[:, p:p + 1])
        for k in ('log_likelihood', 'accuracy'):
            _same(out[k][:, p], one[k], f'{k} of photo {p}')
        for k in ('confidence', 'entropy'):
            _same(out[k], one[k], k)
        assert torch.equal(out['predicted_codes'], one['predicted_codes'])
    assert torch.equal(out['best_camera'].cpu(), _first_argmax(out['log_likelihood']))
    assert torch.equal(out['best_photo'].cpu(), _first_argmax(out['log_likelihood'].transpose(1, 2)))
    # whole views per call: the bits do not depend on the chunking
    for k, v in r.match(q, codes=photos, max_views_per_call=2).items():
        _same_any(v, out[k], f'chunks of 2 views: {k}')
    # context lengths reach the model per camera
    short = r.match(q, codes=photos, n_context=2)
    _same(short['log_likelihood'][:, 0], r.score(q, codes=photos[:, :1], n_context=2)['log_likelihood'], 'n_context = 2')
    assert not torch.equal(short['log_likelihood'], out['log_likelihood'])
    # a planted exact tie: the same camera three times, the same photo four times -> the lowest index, in both directions
    tie = r.match(q[:, [2, 2, 2]], codes=photos[:, [4, 4, 4, 4]])
    assert bool((tie['log_likelihood'] == tie['log_likelihood'][:, :1, :1]).all())
    assert bool((tie['best_camera'] == 0).all()) and bool((tie['best_photo'] == 0).all())
    part = r.match(q[:, [0, 3, 3, 1]], codes=photos[:, [5, 2, 2, 5]])
    assert torch.equal(part['best_camera'].cpu(), _first_argmax(part['log_likelihood']))
    assert torch.equal(part['best_photo'].cpu(), _first_argmax(part['log_likelihood'].transpose(1, 2)))
    assert bool((part['best_camera'] != 2).all()) and bool((part['best_photo'] < 2).all())          # a duplicate never wins over its original
    # a shared photo set (scene axis 1), e.g. a bank's codes
    sh = r.match(q, codes=photos[:1])
    _same(sh['log_likelihood'][0], out['log_likelihood'][0], 'shared photo set, scene 0')
    # images in: each encoded once, the same result as their codes; and the one-call form
    frames, _ = synthetic_scene_batch(B, P_, 32, seed=81)
    frames = torch.from_numpy(frames).to(dev)
    codes = vq.encode(frames.view(-1, 32, 32, 3))[-1].view(B, P_, 8, 8)
    by_img, by_codes = r.match(q, images=frames), r.match(q, codes=codes)
    once = match_views(s.m, vq, None, s.cams[:, :C], q, photos=frames, codes=s.ctx)
    for k in by_img:
        assert torch.equal(by_img[k], by_codes[k]) and torch.equal(by_img[k], once[k]), k
    # M = 0 and P = 0
    e = r.match(q[:, :0], codes=photos)
    assert tuple(e['log_likelihood'].shape) == (B, P_, 0) and tuple(e['best_photo'].shape) == (B, 0) and tuple(e['best_camera'].shape) == (B, P_)
    assert tuple(e['predicted_codes'].shape) == (B, 0, 8, 8)
    e = r.match(q, codes=photos[:, :0])
    assert tuple(e['log_likelihood'].shape) == (B, 0, M_) and tuple(e['accuracy'].shape) == (B, 0, M_)
    assert tuple(e['best_camera'].shape) == (B, 0) and tuple(e['best_photo'].shape) == (B, M_) and e['best_photo'].dtype == torch.int64
    # refusals
    for kw in (dict(), dict(images=frames, codes=photos), dict(codes=photos.float()), dict(codes=photos.bool()), dict(codes=photos.view(B, P_, 64)),
               dict(codes=torch.cat([photos, photos[:1]], 0)), dict(images=frames[0])):
        with pytest.raises(ValueError):
            r.match(q, **kw)
    for qq in (q[:1], q[..., :6]):
        with pytest.raises(ValueError):
            r.match(qq, codes=photos)
