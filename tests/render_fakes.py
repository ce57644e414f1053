"""The stand-ins that ``ViewRenderer`` runs over on the CPU: a transformer, a codebook and the four ``ops`` functions the renderer calls
itself.  Every stand-in answers with a deterministic function of its arguments — a view's "result" depends on its pose, its codes, its
view number, its sample number and its context length — so wrong slicing, order or concatenation in the renderer changes the result; all
of them use sums and products of small dyadic numbers only, which are exact in float32 whatever the CPU.  ``FakeModel.calls`` keeps the
short tuples that the per-method host tests assert on; ``log`` (a callable ``log(name, *args, **kw)``) receives every call in full
(tests/test_view_renderer_calls_host.py).  With ``host`` — a real ``MIGT`` object on the CPU that can own caches — ``prefill_context``
makes a real ``ContextCache`` and the growing calls grow it, so the renderer sees the real ``filled()``, ``alias()``, ``fork()``,
``pack()``, ``lengths`` and ``C``.  No device is touched."""
import numpy as np
import torch


class Cfg:
    token_image_size = 8
    n_embeddings = 128
    augment_poses = 'relative'
    image_size = 32

    def __init__(self, **kw):
        self.__dict__.update(kw)


class FakeCache:
    B = 2


def host_model():
    """a model object on the host that owns caches (tests/test_fork_host.py:_host_model)"""
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    m = MIGT(MIGTConfig(n_embeddings=64, n_head=2, d_model=128, n_layer=2, token_image_size=8, sequence_size=4))
    m.device, m._sd_host = torch.device('cpu'), {}
    m._act_dtypes = lambda: (False, False)
    return m


def _lengths(kw, like):
    """the ``n_context`` keyword of a call as a tensor [B,N] (zeros without one), so that a result depends on it"""
    n = kw.get('n_context')
    return torch.zeros(like.shape[:2], dtype=torch.int64) if n is None else torch.from_numpy(np.asarray(n)).to(torch.int64)


_AXES = torch.tensor([[1., 0, 0, 0], [0, 1., 0, 0], [0, 0, 1., 0], [0, 0, 0, -1.]])


class FakeModel:
    """records what ViewRenderer hands to the ``*_from_context`` methods; a view's answer is a function of its pose, codes, view and
    sample number and context length"""

    def __init__(self, config=None, host=None, log=None):
        self.config = Cfg() if config is None else config
        self.calls, self.host, self.log = [], host, log or (lambda *a, **k: None)

    def _grid(self):
        t = self.config.token_image_size
        return torch.arange(t * t, dtype=torch.int64).view(t, t)

    # ------------------------------------------------------------------ the context
    def prefill_context(self, codes, poses, **kw):
        from viewformer_amd.context_cache import ContextCache, GrowingKVCache
        self.log('prefill_context', codes, poses, **kw)
        m, (B, C), t = self.host, codes.shape[:2], self.config.token_image_size
        d, L, cap = m.config.d_model, t * t, int(kw.get('capacity', C))
        if kw.get('pack') == 'kv':
            bufs = [GrowingKVCache.buffers(B, cap, L, d, torch.float32, m.device) for _ in range(m.config.n_layer)]
            return GrowingKVCache(m, bufs, B, C, (t, t), cap)
        kv = [torch.zeros(B * cap * L, 3 * d) for _ in range(m.config.n_layer)]
        return ContextCache(m, kv, B, C, (t, t), capacity=cap)

    def _grow(self, cache, K):
        if K:
            before = cache.filled()
            cache.reserve(int(before.max()) + K)
            cache.grown(before, K)

    def append_to_context(self, cache, codes, poses):
        self.log('append_to_context', cache, codes, poses)
        self._grow(cache, codes.shape[1])
        return cache

    def rollout_from_context(self, cache, poses, n_samples=1, return_logits=False, fork=False, **kw):
        self.log('rollout_from_context', cache, poses, n_samples=n_samples, return_logits=return_logits, fork=fork, **kw)
        (B, T), S, nE = poses.shape[:2], n_samples, self.config.n_embeddings
        if S > 1:
            cache = cache.fork(S, T) if fork else cache.replicate(S)
        self._grow(cache, T)
        key = (poses * torch.arange(1, 8)).sum(-1).view(B, 1, T, 1, 1)
        codes = ((4 * key).long() + 5 * torch.arange(S).view(1, S, 1, 1, 1) + torch.arange(T).view(1, 1, T, 1, 1) + self._grid()) % nE
        tok = -(codes.float() / 8) - kw.get('seed', 0)
        res = dict(codes=codes, token_log_prob=tok, log_likelihood=tok.sum((3, 4)), cache=cache)
        if return_logits:
            res['logits'] = -(torch.arange(nE) - codes.unsqueeze(-1)).abs().float()
        return res

    def adopt_from_fork(self, parent, child, which, score=None):
        from viewformer_amd.render import choose_best
        self.log('adopt_from_fork', parent, child, which, **({} if score is None else dict(score=score)))
        which = choose_best(score.sum(-1).numpy()) if isinstance(which, str) else np.asarray(which, dtype=np.int64)
        self._grow(parent, int((child.filled() - child.split)[0]))
        return which

    # ------------------------------------------------------------------ the queries
    def generate_from_context(self, cache, poses, codes_only=True, return_confidence=False, **kw):
        self.log('generate_from_context', cache, poses, codes_only=codes_only, return_confidence=return_confidence, **kw)
        (B, N), nE = poses.shape[:2], self.config.n_embeddings
        key = (4 * (poses * torch.arange(1, 8)).sum(-1)).long() + 3 * _lengths(kw, poses)
        codes = (key.view(B, N, 1, 1) + self._grid()) % nE
        if not codes_only:
            return -(torch.arange(nE) - codes.unsqueeze(-1)).abs().float()        # the arg-max of every row is its code
        return (codes, -(codes.float() / 8), codes.float() / 4) if return_confidence else codes

    def sample_from_context(self, cache, poses, n_samples=1, view0=None, **kw):
        self.log('sample_from_context', cache, poses, n_samples=n_samples, **({} if view0 is None else dict(view0=view0)), **kw)
        view0 = view0 or 0                                                       # (the log tells a default from a 0 that was passed)
        self.calls.append((tuple(poses.shape), n_samples, view0, kw))
        (B, N), S, t = poses.shape[:2], n_samples, self.config.token_image_size
        view = (torch.arange(N) + view0).view(1, N, 1, 1, 1) * 10 + torch.arange(S).view(1, 1, S, 1, 1)
        codes = (view + torch.zeros((B, N, S, t, t), dtype=torch.int64))
        tok = codes.float() + poses[..., 0].view(B, N, 1, 1, 1)
        kept = (1 + _lengths(kw, poses)).to(torch.int32).view(B, N, 1, 1).expand(B, N, t, t).contiguous()
        return dict(codes=codes, token_log_prob=tok, log_likelihood=tok.sum((3, 4)), kept=kept)

    def score_from_context(self, cache, poses, codes, **kw):
        self.calls.append((tuple(poses.shape), tuple(codes.shape), kw))
        self.log('score_from_context', cache, poses, codes, **kw)
        return self._score(poses, codes, kw)

    def _score(self, poses, codes, kw):
        (B, N), t = poses.shape[:2], self.config.token_image_size
        c = codes.expand(B, N, t, t).float()
        tok = c + poses[..., 0].view(B, N, 1, 1)
        ent = tok + _lengths(kw, poses).view(B, N, 1, 1)
        return dict(token_log_prob=tok, log_likelihood=tok.sum((2, 3)), predicted_codes=c.long(), confidence=tok, entropy=ent, accuracy=tok.mean((2, 3)))

    def score_grad_from_context(self, cache, poses, codes, **kw):
        self.log('score_grad_from_context', cache, poses, codes, **kw)
        B, N = poses.shape[:2]
        res = self._score(poses, codes, kw)
        res['grad_cameras'] = 2 * poses + codes.expand(B, N, *codes.shape[2:])[:, :, 0, :1].float()
        return res

    def refine_from_context(self, cache, poses, codes, steps=16, return_trace=False, **kw):
        self.log('refine_from_context', cache, poses, codes, steps=steps, return_trace=return_trace, **kw)
        B, N = poses.shape[:2]
        first = codes.expand(B, N, *codes.shape[2:])[:, :, 0, :3].float() / 4 + _lengths(kw, poses).view(B, N, 1)
        ll = first.sum(-1) + poses[..., 0]
        res = dict(cameras=torch.cat((poses[..., :3] + first, poses[..., 3:]), -1), log_likelihood=ll + steps, initial_log_likelihood=ll,
                   accepted=torch.full((B, N), steps, dtype=torch.int32))
        if return_trace:
            res['trace'] = ll.unsqueeze(0) + torch.arange(steps + 1, dtype=torch.float32).view(-1, 1, 1)
        return res

    def match_from_context(self, cache, poses, codes, **kw):
        self.calls.append((tuple(poses.shape), tuple(codes.shape), kw))
        self.log('match_from_context', cache, poses, codes, **kw)
        (B, M), P, t = poses.shape[:2], codes.shape[1], self.config.token_image_size
        key = (4 * (poses * torch.arange(1, 8)).sum(-1)).long() + 3 * _lengths(kw, poses)            # [B,M]
        pred = (key.view(B, M, 1, 1) + self._grid()) % self.config.n_embeddings
        photo = codes.expand(B, P, t, t)[:, :, 0, 0].float()                                         # [B,P]
        m = (-(photo.view(B, 1, P) - key.view(B, M, 1).float() % 16).abs()).transpose(1, 2)          # [B,P,M], a transposed view
        return dict(log_likelihood=m, accuracy=(m / 4).clone(), predicted_codes=pred, confidence=-(pred.float() / 8), entropy=pred.float() / 4)

    def localize_from_context(self, cache, codes, return_tokens=False, **kw):
        self.log('localize_from_context', cache, codes, return_tokens=return_tokens, **kw)
        (B, N), L = codes.shape[:2], self.config.token_image_size ** 2
        row = codes[:, :, 0].to(torch.int64)
        cams = torch.cat((row[:, :, :3].float() / 4 + _lengths(kw, codes).view(B, N, 1), _AXES[row[:, :, 3] % 4]), -1)
        if not return_tokens:
            return cams
        per_token = cams.view(B, N, 1, 7) + torch.zeros(B, N, L, 7)
        return dict(cameras=cams, pose_prediction=per_token, raw=per_token * 2)


class FakeCodebook:
    device = torch.device('cpu')
    data_format = 'NHWC'

    def __init__(self, config=None, log=None):
        self.config = Cfg() if config is None else config
        self.encoded, self.log = 0, log or (lambda *a, **k: None)

    def encode(self, frames):
        self.encoded += frames.shape[0]
        self.log('encode', frames)
        t = self.config.token_image_size
        return (None, frames.reshape(frames.shape[0], -1)[:, :t * t].to(torch.int32).view(-1, t, t))

    def decode_code(self, flat):
        self.log('decode_code', flat)
        s = self.config.image_size // self.config.token_image_size
        up = flat.float().repeat_interleave(s, 1).repeat_interleave(s, 2)
        return torch.stack((up, up + 1, up + 2), -1)


def fake_ops(log):
    """CPU stand-ins for the ``ops`` functions the renderer calls itself, by name"""
    def postprocess_u8(dec):
        log('postprocess_u8', dec)
        return dec.to(torch.uint8)

    def argmax_rows(x, rows, n):                                               # the first maximum of every row
        log('argmax_rows', x, rows, n)
        x = x.reshape(rows, n)
        at = torch.where(x == x.max(-1, keepdim=True).values, torch.arange(n), n)
        return at.min(-1).values

    def logits_score(x, rows, n, want=()):
        log('logits_score', x, rows, n, want=want)
        x = x.reshape(rows, n)
        full = dict(max_logit=x.max(-1).values, lse=x.max(-1).values + 2, entropy=-x.min(-1).values / 4)
        return {k: full[k] for k in want}

    def resize_u8(flat, size):
        log('resize_u8', flat, size)
        return flat[:, ::flat.shape[1] // size, ::flat.shape[2] // size].contiguous()

    return dict(postprocess_u8=postprocess_u8, argmax_rows=argmax_rows, logits_score=logits_score, resize_u8=resize_u8)
