"""GPU: mean views from a context cache (MIGT.expect_from_context, ViewRenderer.render_mean, render.mean_views) on the tiny model of
tests/test_hip_sample.py, both arms.  Every comparison is ``torch.equal``: the model's latents against ops.mix_rows on the logits of
``generate_from_context(codes_only=False)``; ``top_k = 1`` against the codebook's columns of the generated codes and against ``render``'s
images; a view's result across N, the chunking and ``n_context``; a forked, a K/V-only and an e4m3 cache against their plain copies; the
one-call form.  Last, on the tiny model trained until its logits are peaked: the PSNR of the arg-max view and of the mean view against
the photo the context does not hold — recorded, not asserted (nobody has measured which is higher)."""
import numpy as np
import pytest
import torch

import test_hip_sample as GS
from conftest import parity_report

pytestmark = pytest.mark.gpu

B_, C_, N_, L_ = GS.B_, GS.C_, GS.N_, GS.L_
KW = dict(temperature=0.8, top_k=32, top_p=0.9)
_vq = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _codebook(dev):
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_vqgan_weights
    if 'vq' not in _vq:
        vcfg = VQGANConfig(**GS.SMALL_VQ)
        _vq['vq'] = VQGAN(vcfg, data_format='NHWC').load_state_dict(make_vqgan_weights(vcfg, seed=1, codebook_scale=0.05)).to(dev)
    return _vq['vq']


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _equal(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f'{what}: {k} differs in its bits'


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_expect_from_context_is_mix_rows_on_the_logits(dev, arm):
    from viewformer_amd import ops
    s, vq = GS._setup(dev, arm), _codebook(dev)
    E = vq.codebook_embedding()
    nE, D = s.cfg.n_embeddings, E.shape[0]
    assert E.data_ptr() == vq._E.data_ptr() and tuple(E.shape) == (32, 128) and E.dtype == torch.float32       # the tensor itself
    M = B_ * N_ * L_
    for kw in (dict(), KW, dict(temperature=2.0, top_p=0.5)):
        out = s.m.expect_from_context(s.cache, s.qpos, E, **kw)
        assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == dict(latents=((B_, N_, 8, 8, D), torch.float32),
                                                                              kept=((B_, N_, 8, 8), torch.int32))
        want = ops.mix_rows(s.lg.view(-1, nE), M, nE, E, D, want=('out', 'kept'), **kw)
        assert torch.equal(_bits(out['latents'].reshape(M, D)), _bits(want['out'])) and torch.equal(out['kept'].reshape(M), want['kept'])
        smp = s.m.sample_from_context(s.cache, s.qpos, **kw)
        assert torch.equal(out['kept'], smp['kept'])                                # the set sample_from_context draws from
    assert bool((s.m.expect_from_context(s.cache, s.qpos, E)['kept'] == nE).all())   # no filter: every code
    # N = 0
    empty = s.m.expect_from_context(s.cache, s.qpos[:, :0], E)
    assert {k: (tuple(v.shape), v.dtype) for k, v in empty.items()} == dict(latents=((B_, 0, 8, 8, D), torch.float32), kept=((B_, 0, 8, 8), torch.int32))
    # refusals, before any launch
    for bad in (E[:, :64].contiguous(), E[:16].contiguous(), E.double(), E.t(), E.cpu(), None):      # (a host embedding: before the transformer runs)
        with pytest.raises(ValueError):
            s.m.expect_from_context(s.cache, s.qpos, bad)
    for kw in (dict(temperature=0.0), dict(top_p=float('nan')), dict(top_k=-1), dict(top_k=1.5)):
        with pytest.raises(ValueError):
            s.m.expect_from_context(s.cache, s.qpos, E, **kw)
    with pytest.raises(ValueError):
        s.m.expect_from_context(s.cache, s.qpos[:1], E)


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_top_k_1_is_the_generated_view(dev, arm):
    from viewformer_amd import ops
    from viewformer_amd.render import ViewRenderer, query_poses
    s, vq = GS._setup(dev, arm), _codebook(dev)
    E = vq.codebook_embedding()
    out = s.m.expect_from_context(s.cache, s.qpos, E, top_k=1)
    assert int(out['kept'].max()) == 1                                              # every token of this model has a unique maximum
    gen = s.m.generate_from_context(s.cache, s.qpos)
    want = ops.codebook_gather(E, gen.reshape(-1), E.shape[0], E.shape[1])
    assert torch.equal(_bits(out['latents'].reshape(-1, E.shape[0])), _bits(want))
    r = ViewRenderer(s.m, vq).set_context(codes=s.ctx, cameras=s.cams[:, :C_])
    q = s.cams[:, C_:].to(dev)
    before = r.render(q, return_codes=True)
    mean = r.render_mean(q, top_k=1, return_latents=True)
    assert torch.equal(mean['generated_images'], before['generated_images'])
    assert torch.equal(_bits(mean['decoded']), _bits(before['decoded'])) and int(mean['kept'].max()) == 1
    # the renderer's poses are the model's, and render is what it was
    direct = s.m.expect_from_context(r.cache, query_poses(q, r.transform), E, top_k=1)
    assert torch.equal(_bits(direct['latents']), _bits(mean['latents']))
    _equal(r.render(q, return_codes=True), before, 'render after render_mean')


@pytest.mark.parametrize('arm', ['bf16', 'f32'])
def test_a_views_result_depends_on_nothing_but_the_view(dev, arm):
    from viewformer_amd import ops
    from viewformer_amd.render import ViewRenderer, mean_views
    s, vq = GS._setup(dev, arm), _codebook(dev)
    r = ViewRenderer(s.m, vq).set_context(codes=s.ctx, cameras=s.cams[:, :C_])
    q = s.cams[:, C_:].to(dev)
    one = r.render_mean(q, return_latents=True, **KW)
    assert {k: (tuple(v.shape), v.dtype) for k, v in one.items()} == dict(
        generated_images=((B_, N_, 32, 32, 3), torch.uint8), kept=((B_, N_, 8, 8), torch.int32),
        latents=((B_, N_, 8, 8, 32), torch.float32), decoded=((B_, N_, 32, 32, 3), torch.float32))
    assert set(r.render_mean(q)) == {'generated_images', 'kept'}
    for cap in (1, 3):                                                              # the chunking
        _equal(r.render_mean(q, max_views_per_call=cap, return_latents=True, **KW), one, f'max_views_per_call {cap}')
    for a, b in ((0, 1), (2, 7)):                                                   # N
        _equal(r.render_mean(q[:, a:b], return_latents=True, **KW), {k: v[:, a:b] for k, v in one.items()}, f'views {a}:{b}')
    alone = ViewRenderer(s.m, vq).set_context(codes=s.ctx[1:], cameras=s.cams[1:, :C_]).render_mean(q[1:], return_latents=True, **KW)
    _equal(alone, {k: v[1:] for k, v in one.items()}, 'scene 1 alone')              # the other scenes of the batch
    # n_context = c against a cache of c views
    for c in (1, 2):
        short = ViewRenderer(s.m, vq).set_context(codes=s.ctx[:, :c], cameras=s.cams[:, :c])
        _equal(r.render_mean(q, n_context=c, return_latents=True, **KW), short.render_mean(q, return_latents=True, **KW), f'n_context {c}')
    lens = np.array([[0, 1, 2, 3, 3, 2, 1, 0], [3, 3, 0, 0, 1, 1, 2, 2]])
    ragged = r.render_mean(q, n_context=lens, return_latents=True, **KW)
    _equal(r.render_mean(q, n_context=lens, max_views_per_call=3, return_latents=True, **KW), ragged, 'ragged lengths, chunked')
    assert torch.equal(ragged['latents'][lens == 3], one['latents'][lens == 3])
    # the images are the decoder's output of the latents
    dec = vq.decode(one['latents'][1, 5][None]).contiguous()
    assert torch.equal(ops.postprocess_u8(dec)[0], one['generated_images'][1, 5])
    # the one-call form
    _equal(mean_views(s.m, vq, None, s.cams[:, :C_], q, codes=s.ctx, return_latents=True, **KW), one, 'mean_views')
    # N = 0
    empty = r.render_mean(q[:, :0], return_latents=True)
    assert tuple(empty['generated_images'].shape) == (B_, 0, 32, 32, 3) and tuple(empty['latents'].shape) == (B_, 0, 8, 8, 32)


@pytest.mark.parametrize('form', ['fork', 'kv bf16', 'kv f32', 'e4m3', 'growing'])
def test_every_cache_form_answers_as_its_plain_copy(dev, form):
    arm = 'f32' if form == 'kv f32' else 'bf16'
    s, vq = GS._setup(dev, arm), _codebook(dev)
    E, m, q = vq.codebook_embedding(), s.m, s.qpos[:, :3].contiguous()
    if form == 'fork':
        cache = s.cache.fork(2)
        plain, q = cache.materialize(), q.repeat_interleave(2, 0).contiguous()
        assert cache.forked() and not plain.forked()
    elif form == 'e4m3':
        cache = s.cache.pack('e4m3')
        plain = cache.unpack()
        assert cache.packed == 'e4m3' and plain.packed is None
    elif form == 'growing':
        cache = m.prefill_context(s.ctx[:, :2], s.cpos[:, :2].contiguous(), capacity=4)
        m.append_to_context(cache, s.ctx[:, 2:], s.cpos[:, 2:].contiguous())
        plain = s.cache
        assert cache.capacity == 4 and cache.filled().tolist() == [C_] * B_
    else:
        cache = s.cache.pack()
        plain = cache.unpack()
        assert cache.packed == 'kv' and plain.packed is None
    for kw in (KW, dict(n_context=2, **KW)):
        a, b = m.expect_from_context(cache, q, E, **kw), m.expect_from_context(plain, q, E, **kw)
        if form == 'growing':                     # an appended view's keys come from the prefix kernel, a prefilled view's from the block-causal
            assert tuple(a['latents'].shape) == tuple(b['latents'].shape) and bool(torch.isfinite(a['latents']).all())      # one: the arm's own error apart
            if 'n_context' in kw:
                _equal(a, b, f'{form} {sorted(kw)}')                                # the two prefilled views: the same rows
        else:
            _equal(a, b, f'{form} {sorted(kw)}')


def _psnr(a, b):
    mse = (a.float() - b.float()).pow(2).mean((-3, -2, -1))
    return (10 * torch.log10(255.0 ** 2 / mse.clamp_min(1e-12))).cpu().tolist()


def test_psnr_of_the_argmax_view_and_of_the_mean_view_is_recorded(dev):
    """the tiny model trained as tests/test_hip_score_grad.py trains it (8 scenes of 5 views, 300 steps), a context of each scene's first 4
    views, the query at the fifth view's camera: PSNR of ``render`` and of ``render_mean`` (T = 1; top_p = 0.9) against the fifth
    photograph, per scene.  Recorded, not asserted."""
    import test_hip_score_grad as SG
    from viewformer_amd.render import ViewRenderer
    from viewformer_amd.weights import synthetic_scene_batch
    s, vq = SG._trained_setup(dev, 'bf16'), _codebook(dev)
    frames, cams = synthetic_scene_batch(8, 5, 32, seed=33)
    photo = torch.from_numpy(frames[:, 4]).to(dev)
    t = SG._trained
    # the photographs re-made here are the ones the model was trained on: their codes are the trainer's
    again = vq.encode(torch.from_numpy(frames.reshape(-1, 32, 32, 3)).to(dev))[-1].view(8, 5, 8, 8)
    assert torch.equal(again.to(torch.int32), t['codes'].to(dev))
    r = ViewRenderer(s.m, vq).set_context(codes=t['codes'][:, :4], cameras=torch.from_numpy(cams[:, :4]))
    q = torch.from_numpy(cams[:, 4:5]).to(dev)
    arg = r.render(q)['generated_images'][:, 0]
    mean = r.render_mean(q)
    nucleus = r.render_mean(q, top_p=0.9)
    rec = dict(argmax=_psnr(arg, photo), mean_T1=_psnr(mean['generated_images'][:, 0], photo), mean_top_p_09=_psnr(nucleus['generated_images'][:, 0], photo))
    parity_report(test='mean_views_psnr', trained_ce=s.ce, kept_top_p_09=float(nucleus['kept'].float().mean()),
                  **{k: [round(x, 3) for x in v] for k, v in rec.items()})
    assert all(len(v) == 8 and all(np.isfinite(v)) for v in rec.values())
    assert tuple(mean['generated_images'].shape) == (8, 1, 32, 32, 3)
