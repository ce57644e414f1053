"""CPU: the host plumbing of ``ViewRenderer.render_mean`` / ``render.mean_views`` over the stand-ins of tests/render_fakes.py — the call
sequence (one ``expect_from_context`` per chunk of whole views with the cameras in the context's frame and the codebook's own embedding
tensor, one ``decode`` per MAX_SCENES_PER_CALL views, one ``postprocess_u8`` per decode), the shapes, the chunking, N = 0 and every refusal
before any call.  The stand-ins answer with exact functions of their arguments; the expectations are written inline.  No device is
touched."""
import numpy as np
import pytest
import torch

import render_fakes as F
from training_kernels_ref import rng

B, N, T_IMG, D, SIZE = 2, 8, 8, 4, 32
EMB = torch.arange(D * 128, dtype=torch.float32).view(D, 128)


class Cache(F.FakeCache):
    C = 3


class Model(F.FakeModel):
    """+ ``expect_from_context``: latents[b,n,y,x,d] = 8 * (view's pose x) + the token's number / 64 + d + 4 * its context length"""

    def expect_from_context(self, cache, poses, embedding, **kw):
        self.log('expect_from_context', cache, poses, embedding, **kw)
        self.calls.append((tuple(poses.shape), embedding, kw))
        (b, n), t = poses.shape[:2], self.config.token_image_size
        lens = F._lengths(kw, poses)
        lat = (8 * poses[..., 0].view(b, n, 1, 1, 1) + self._grid().view(1, 1, t, t, 1) / 64 + torch.arange(D).view(1, 1, 1, 1, D)
               + 4 * lens.view(b, n, 1, 1, 1))
        return dict(latents=lat, kept=(1 + lens).to(torch.int32).view(b, n, 1, 1).expand(b, n, t, t).contiguous())


class Codebook(F.FakeCodebook):
    """+ ``codebook_embedding`` and ``decode``: the first three latent features of a token fill its patch of the image"""

    def __init__(self, data_format='NHWC', **kw):
        super().__init__(**kw)
        self.data_format, self.decoded = data_format, []

    def codebook_embedding(self):
        return EMB

    def decode(self, quant):
        self.log('decode', quant)
        self.decoded.append(tuple(quant.shape))
        q = quant.permute(0, 2, 3, 1) if self.data_format == 'NCHW' else quant
        s = self.config.image_size // self.config.token_image_size
        up = q[..., :3].repeat_interleave(s, 1).repeat_interleave(s, 2)
        return up.permute(0, 3, 1, 2) if self.data_format == 'NCHW' else up


@pytest.fixture
def posted(monkeypatch):
    from viewformer_amd import ops
    seen = []
    monkeypatch.setattr(ops, 'postprocess_u8', lambda dec: (seen.append((tuple(dec.shape), dec.is_contiguous())), dec.to(torch.uint8))[1])
    return seen


def _renderer(data_format='NHWC'):
    from viewformer_amd.render import ViewRenderer
    r = ViewRenderer(Model(), Codebook(data_format))
    r.cache = Cache()
    r.transform = torch.from_numpy(rng(7).standard_normal((B, 1, 7)).astype(np.float32))
    return r


def _cameras(n=N):
    return torch.from_numpy(rng(8).standard_normal((B, n, 7)).astype(np.float32))


def test_render_mean_calls_the_model_once_per_chunk_and_the_decoder_once(posted):
    from viewformer_amd.render import query_poses
    q, r = _cameras(), _renderer()
    out = r.render_mean(q, temperature=0.7, top_k=5, top_p=0.9)
    assert list(out) == ['generated_images', 'kept']
    assert len(r.transformer.calls) == 1
    shape, emb, kw = r.transformer.calls[0]
    assert shape == (B, N, 7) and emb is EMB and kw == dict(temperature=0.7, top_k=5, top_p=0.9)      # the codebook's tensor itself, no copy
    assert r.codebook.decoded == [(B * N, T_IMG, T_IMG, D)] and posted == [((B * N, SIZE, SIZE, 3), True)]
    assert tuple(out['generated_images'].shape) == (B, N, SIZE, SIZE, 3) and out['generated_images'].dtype == torch.uint8
    assert tuple(out['kept'].shape) == (B, N, T_IMG, T_IMG) and out['kept'].dtype == torch.int32 and bool((out['kept'] == 1).all())
    # the cameras reach the model in the context's frame, and the image is the decoder's output of the latents
    full = r.render_mean(q, return_latents=True)
    assert list(full) == ['generated_images', 'kept', 'latents', 'decoded']
    pose_x = query_poses(q, r.transform)[..., 0]
    grid = torch.arange(T_IMG * T_IMG).view(T_IMG, T_IMG) / 64
    want = 8 * pose_x.view(B, N, 1, 1, 1) + grid.view(1, 1, T_IMG, T_IMG, 1) + torch.arange(D).view(1, 1, 1, 1, D)
    assert torch.equal(full['latents'], want) and tuple(full['latents'].shape) == (B, N, T_IMG, T_IMG, D)
    s = SIZE // T_IMG
    dec = want[..., :3].repeat_interleave(s, 2).repeat_interleave(s, 3)
    assert torch.equal(full['decoded'], dec) and torch.equal(full['generated_images'], dec.to(torch.uint8))
    # defaults
    assert r.transformer.calls[-1][2] == dict(temperature=1.0, top_k=0, top_p=1.0)


def test_a_views_result_does_not_depend_on_the_chunking(posted):
    q = _cameras()
    one = _renderer().render_mean(q, top_p=0.5, return_latents=True)
    r = _renderer()
    parts = r.render_mean(q, top_p=0.5, max_views_per_call=3, return_latents=True)
    assert [c[0] for c in r.transformer.calls] == [(B, 3, 7), (B, 3, 7), (B, 2, 7)]
    assert r.codebook.decoded == [(B * N, T_IMG, T_IMG, D)]                             # the decoder's chunks are its own: MAX_SCENES_PER_CALL views
    for k in one:
        assert torch.equal(one[k], parts[k]), k
    # the context lengths are sliced with the views
    lens = np.array([[0, 1, 2, 3, 3, 2, 1, 0], [3, 3, 3, 0, 0, 0, 1, 2]])
    r = _renderer()
    a = r.render_mean(q, n_context=lens, max_views_per_call=5)
    assert [c[2]['n_context'].tolist() for c in r.transformer.calls] == [lens[:, :5].tolist(), lens[:, 5:].tolist()]
    assert torch.equal(a['kept'][:, :, 0, 0], torch.from_numpy(1 + lens).to(torch.int32))
    b = _renderer().render_mean(q, n_context=lens)
    assert torch.equal(a['generated_images'], b['generated_images'])


def test_the_decoder_is_walked_in_its_own_chunks_and_in_its_data_format(posted, monkeypatch):
    from viewformer_amd import render
    monkeypatch.setattr(render, 'MAX_SCENES_PER_CALL', 6)
    q = _cameras()
    r = _renderer('NCHW')
    got = r.render_mean(q, return_latents=True)
    assert r.codebook.decoded == [(6, D, T_IMG, T_IMG), (6, D, T_IMG, T_IMG), (4, D, T_IMG, T_IMG)]
    assert posted == [((6, SIZE, SIZE, 3), True), (((6, SIZE, SIZE, 3)), True), ((4, SIZE, SIZE, 3), True)]
    posted.clear()
    want = _renderer('NHWC').render_mean(q, max_views_per_call=8, return_latents=True)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_no_views_no_launch(posted):
    r = _renderer()
    out = r.render_mean(_cameras(0), return_latents=True)
    assert [c[0] for c in r.transformer.calls] == [(B, 0, 7)] and 'n_context' not in r.transformer.calls[0][2]      # the empties' shapes: the model's
    assert r.codebook.decoded == [] and posted == []
    assert tuple(out['generated_images'].shape) == (B, 0, SIZE, SIZE, 3) and out['generated_images'].dtype == torch.uint8
    assert tuple(out['kept'].shape) == (B, 0, T_IMG, T_IMG) and tuple(out['latents'].shape) == (B, 0, T_IMG, T_IMG, D)
    assert tuple(out['decoded'].shape) == (B, 0, SIZE, SIZE, 3) and out['decoded'].dtype == torch.float32


def test_every_refusal_comes_before_any_call(posted):
    from viewformer_amd.render import ViewRenderer
    q = _cameras()
    with pytest.raises(RuntimeError):
        ViewRenderer(Model(), Codebook()).render_mean(q)                              # no context
    r = _renderer()
    for bad in (q[:1], torch.zeros((B, 4, 6)), torch.zeros((B, 7))):                    # another batch size, not 7 numbers, no view axis
        with pytest.raises(ValueError):
            r.render_mean(bad)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('inf')), dict(temperature=float('nan')), dict(top_p=0.0),
               dict(top_p=-0.1), dict(top_p=float('nan')), dict(top_k=-1), dict(top_k=1.5), dict(top_k=True), dict(max_views_per_call=0), dict(n_context=4),
               dict(n_context=np.zeros((B, N + 1), dtype=np.int64))):
        with pytest.raises(ValueError):
            r.render_mean(q, **kw)
    plain = ViewRenderer(Model(), F.FakeCodebook())                                    # a codebook without codebook_embedding
    plain.cache, plain.transform = Cache(), None
    with pytest.raises(TypeError, match='codebook_embedding'):
        plain.render_mean(q)
    assert r.transformer.calls == [] and plain.transformer.calls == [] and r.codebook.decoded == [] and posted == []


def test_the_model_refuses_an_embedding_it_cannot_mix_before_any_launch():
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    m = MIGT(MIGTConfig(sequence_size=3, n_layer=1, n_embeddings=128))
    q = torch.zeros((B, 4, 7))
    for emb in (torch.zeros(32, 64), torch.zeros(48, 128), torch.zeros(288, 128), torch.zeros(128), torch.zeros(32, 128, dtype=torch.float64), None):
        with pytest.raises(ValueError):
            m.expect_from_context(Cache(), q, emb)
    for kw in (dict(temperature=0.0), dict(top_p=0.0), dict(top_k=-1)):
        with pytest.raises(ValueError):
            m.expect_from_context(Cache(), q, torch.zeros(32, 128), **kw)
    for kw in (dict(top_k=1.5), dict(top_k=True)):                                     # nothing is truncated on the caller's behalf
        with pytest.raises(ValueError):
            m.expect_from_context(Cache(), q, torch.zeros(32, 128), **kw)
    with pytest.raises(TypeError):
        m.expect_from_context(Cache(), q, torch.zeros(32, 128))                        # not a ContextCache of prefill_context
    host = F.host_model()                                                              # a model that lives somewhere: the embedding must live there too
    with pytest.raises(ValueError, match='lives on'):
        host.expect_from_context(Cache(), q, torch.zeros(32, 64, device='meta'))


def test_mean_views_is_the_one_call_form(posted, monkeypatch):
    from viewformer_amd import ops, render
    for name, fn in F.fake_ops(lambda *a, **k: None).items():
        if name != 'postprocess_u8':
            monkeypatch.setattr(ops, name, fn)
    cfg = F.Cfg(n_embeddings=64)
    codes = (torch.arange(B * 3 * T_IMG * T_IMG).view(B, 3, T_IMG, T_IMG) % 64).to(torch.int64)
    cams = torch.from_numpy(rng(9).standard_normal((B, 3, 7)).astype(np.float32))
    cams[..., 3:] = torch.tensor([1.0, 0, 0, 0])
    q = _cameras()
    q[..., 3:] = torch.tensor([0, 1.0, 0, 0])
    tm, cm = Model(cfg, F.host_model()), Codebook(config=cfg)
    one = render.mean_views(tm, cm, None, cams, q, codes=codes, top_p=0.9, max_views_per_call=5, return_latents=True)
    assert [c[0] for c in tm.calls] == [(B, 5, 7), (B, 3, 7)] and tm.calls[0][2] == dict(temperature=1.0, top_k=0, top_p=0.9)
    r = render.ViewRenderer(Model(cfg, F.host_model()), Codebook(config=cfg)).set_context(codes=codes, cameras=cams)
    two = r.render_mean(q, top_p=0.9, return_latents=True)
    for k in two:
        assert torch.equal(one[k], two[k]), k
