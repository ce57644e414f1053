"""CPU: the launch sequences of the context cache, form by form.  Every ``ops`` function the cached-context methods
call, and ``MIGT._dense_launch`` / ``_gemm``, is replaced by a recorder that returns correctly shaped CPU tensors and writes down, per
call, the function's name and every argument: a tensor as 'dtype[shape]/[stride]+storage offset#the number of its storage among the
buffers seen so far in the sequence' (small int32 tensors with '=their values'), a scalar as it is.  The sequences of ``generate`` on every
storage form, ``append`` on a plain and on a forked cache, roll-out steps, ``materialize``, ``pack``, ``unpack`` and ``adopt_from_fork``
must equal ``tests/golden/context_cache_launches.json``, recorded before the cache forms became classes of their own: a launch whose
stride, offset or buffer moved would read another scene's keys on the device.  The fixture keeps every call as 'name:digest' (the first
12 hex digits of the SHA-256 of the call's arguments as JSON) and every resulting cache's state in full; a call that differs is reported
with its live arguments.  No device is touched.

``python tests/test_context_cache_launches_host.py`` prints the fixture of the code as it stands, ``... --full`` every call with its
arguments, one per line, for a diff between two checkouts."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'context_cache_launches.json')
B, C0, CAP, N, S, T, L, D, H, NE, NL = 2, 3, 5, 5, 2, 2, 64, 128, 2, 64, 2
LENGTHS = [2, 3]


class Recorder:
    def __init__(self):
        self.calls, self.buffers, self.keep = [], {}, []

    def reset(self):
        self.calls, self.buffers = [], {}

    def arg(self, x):
        if isinstance(x, torch.Tensor):
            st = x.untyped_storage()
            self.keep.append(x)                                                # alive: a freed buffer's address would come back as another's
            buf = -1 if st.nbytes() == 0 else self.buffers.setdefault(st.data_ptr(), len(self.buffers))
            r = '%s%s/%s+%d#%d' % (str(x.dtype)[6:], list(x.shape), list(x.stride()), x.storage_offset(), buf)
            return (r + '=%s' % x.reshape(-1).tolist() if x.dtype == torch.int32 and x.numel() <= 64 else r).replace(' ', '')
        if isinstance(x, (tuple, list)):
            return [self.arg(y) for y in x]
        if isinstance(x, (np.integer, np.floating)):
            return x.item()
        assert x is None or isinstance(x, (bool, int, float, str)), type(x)
        return x

    def wrap(self, name, result=lambda *a, **k: None):
        def fn(*a, **k):
            self.calls.append([name] + [self.arg(x) for x in a] + [{n: self.arg(k[n]) for n in sorted(k)}] * bool(k))
            return result(*a, **k)
        return fn


def _sample_rows(lg, rows, n, n_samples=1, want=('idx', 'logp'), **kw):
    full = dict(idx=torch.zeros((rows, n_samples), dtype=torch.int64), logp=torch.zeros((rows, n_samples)),
                kept=torch.zeros(rows, dtype=torch.int32))
    return {k: full[k] for k in want}


def host_records(m, shapes, tensors=True):
    """``m._dense`` and ``m._head`` for layers of ``shapes`` = {name: (k, n)} without an upload: records that hold no packing (every
    launch that would read one is a recorder's), with zero weights and biases, or none where the caller binds its own"""
    from viewformer_amd.migt import _Dense
    for name, (k, n) in shapes.items():
        m._dense[name] = _Dense(k, n, torch.zeros(k, n), torch.zeros(n)) if tensors else _Dense(k, n)
    m._head = _Dense(m.config.d_model, m.config.n_embeddings)


def _model(monkeypatch, rec, arm):
    """the host model of tests/test_fork_host.py with fake weights, every launch a recorder"""
    from viewformer_amd import ops
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    m = MIGT(MIGTConfig(n_embeddings=NE, n_head=H, d_model=D, n_layer=NL, token_image_size=8, sequence_size=4), precision=arm)
    m.device, m._sd_host = torch.device('cpu'), {}
    lp = arm == 'bf16'
    m._act_dtypes = lambda: (lp, lp)
    shapes = {'pose_embedding.c_fc': (7, 4 * D), 'pose_embedding.c_proj': (4 * D, D)}
    for i in range(NL):
        shapes.update({f'h.{i}.attn.c_attn': (D, 3 * D), f'h.{i}.attn.c_proj': (D, D), f'h.{i}.mlp.c_fc': (D, 4 * D), f'h.{i}.mlp.c_proj': (4 * D, D)})
        m._ln[f'h.{i}.ln_1'] = (torch.zeros(D), torch.zeros(D)); m._ln[f'h.{i}.ln_2'] = (torch.zeros(D), torch.zeros(D))
    host_records(m, shapes)
    m._ln['ln_f'] = (torch.zeros(D), torch.zeros(D))
    m._wte, m._wpe, m._head.packed['f32'] = torch.zeros(NE + 2, D), torch.zeros(L, D), torch.zeros(NE, D)
    names = {id(d): n for n, d in m._dense.items()}
    m._dense_launch = rec.wrap('_dense_launch')
    m._dense_launch = (lambda f: lambda x, d, *a, **k: f(x, names[id(d)], *a, **k))(m._dense_launch)
    m._gemm = rec.wrap('_gemm', lambda x, name, M, epilogue=None, res=None, out_bf16=False:
                       torch.zeros((M, m._dense[name].n), dtype=torch.bfloat16 if out_bf16 else torch.float32))
    stubs = dict(
        embed_sum=lambda ids, wte, wpe, add, BS, L_, d, vocab: torch.zeros(BS * L_, d),
        layernorm=lambda x, g, b, rows, d, out_bf16=False: torch.zeros(x.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32),
        dense_small_k=lambda x, W, b, rows, K, n, gelu: torch.zeros(rows, n),
        argmax_rows=lambda x, rows, n: torch.zeros(rows, dtype=torch.int64),
        sample_rows=_sample_rows,
        sample_views=lambda logp, views, L_, S_: torch.zeros(views, S_))
    for name in ('kv_append', 'attn_prefix', 'attn_prefix_fork', 'attn_prefix_q8', 'kv_pack_e4m3', 'igemm'):
        stubs[name] = lambda *a, **k: None
    for name, fn in stubs.items():
        monkeypatch.setattr(ops, name, rec.wrap(name, fn))
    igemm = ops.igemm                                          # an arm keyword left out is that keyword passed as False: the same launch
    monkeypatch.setattr(ops, 'igemm', lambda *a, **k: igemm(*a, **dict(dict(bf16=False, x6=False, x3h=False), **k)))
    return m


def _state(c):
    """what a cache says about itself, for the sequences that end in a new or a grown cache"""
    shapes = [[list(x.shape) + [str(x.dtype)] for x in (t if isinstance(t, (tuple, list)) else (t,))] for t in c.kv]
    st = dict(B=c.B, C=c.C, capacity=c.capacity, lengths=None if c.lengths is None else c.lengths.tolist(), filled=c.filled().tolist(),
              ragged=bool(c.ragged()), forked=bool(c.forked()), packed=c.packed, kv=shapes, nbytes=c.nbytes())
    if c.forked():
        st.update(split=c.split.tolist(), share=c.share, room=c.room, parent_capacity=c.parent_capacity,
                  parent_kv=[list(x.shape) for x in c.parent_kv])
    return st


def record(monkeypatch, arm):
    from viewformer_amd.migt import ContextCache
    rec = Recorder()
    m = _model(monkeypatch, rec, arm)
    dt = torch.bfloat16 if arm == 'bf16' else torch.float32
    out = {}

    def seq(name, fn, state=None):
        rec.reset()
        res = fn()
        out[name] = dict(calls=rec.calls)
        if state is not None:
            out[name]['cache'] = _state(state(res))
        return res

    def tight():
        return ContextCache(m, [torch.zeros(B * C0 * L, 3 * D, dtype=dt) for _ in range(NL)], B, C0, (8, 8))

    def slack():
        return ContextCache(m, [torch.zeros(B * CAP * L, 3 * D, dtype=dt) for _ in range(NL)], B, C0, (8, 8), capacity=CAP, lengths=LENGTHS)

    cams = lambda b, n: torch.zeros(b, n, 7)
    codes = lambda b, n: torch.zeros(b, n, 8, 8, dtype=torch.int64)
    same = lambda c: (lambda res: c)
    forms = dict(tight=tight(), slack=slack())
    forms['fork'] = seq('fork', lambda: slack().fork(S, room=1), state=lambda c: c)
    forms['kv'] = seq('pack_kv', lambda: slack().pack(None), state=lambda c: c)
    if arm == 'bf16':
        forms['e4m3'] = seq('pack_e4m3', lambda: slack().pack('e4m3'), state=lambda c: c)
    for form, c in forms.items():
        seq('generate_' + form, lambda: m.generate_from_context(c, cams(c.B, N)))
        if c.packed:
            seq('unpack_' + form, c.unpack, state=lambda c: c)
    c = slack()
    seq('append_plain_fits', lambda: m.append_to_context(c, codes(B, 2), cams(B, 2)), state=same(c))
    seq('append_plain_grows', lambda: m.append_to_context(c, codes(B, 1), cams(B, 1)), state=same(c))
    parent = slack()
    f = parent.fork(S, room=1)
    seq('append_fork_fits', lambda: m.append_to_context(f, codes(B * S, 1), cams(B * S, 1)), state=same(f))
    seq('append_fork_grows', lambda: m.append_to_context(f, codes(B * S, 1), cams(B * S, 1)), state=same(f))
    seq('generate_fork_grown', lambda: m.generate_from_context(f, cams(B * S, N), n_context=[3, 4, 2, 5]))
    seq('materialize_fork', f.materialize, state=lambda c: c)
    seq('materialize_plain', parent.materialize, state=lambda c: c)
    seq('adopt_from_fork', lambda: m.adopt_from_fork(parent, f, [1, 0]), state=same(parent))
    seq('replicate', lambda: m._replicate(slack(), S), state=lambda c: c)
    for name, kw in (('rollout_fused', {}), ('rollout_unfused', dict(fused_step=False)), ('rollout_fork', dict(n_samples=S, fork=True))):
        seq(name, lambda: m.rollout_from_context(slack(), cams(B, T), top_k=0, seed=3, **kw), state=lambda r: r['cache'])
    return out


def digest(call):
    return call[0] + ':' + hashlib.sha256(json.dumps(call[1:], separators=(',', ':'), sort_keys=True).encode()).hexdigest()[:12]


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_every_form_issues_the_recorded_launches(monkeypatch, arm):
    got = json.loads(json.dumps(record(monkeypatch, arm)))
    with open(GOLDEN) as fh:
        want = json.load(fh)[arm]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].get('cache') == want[name].get('cache'), name
        assert len(got[name]['calls']) == len(want[name]['calls']), name
        for i, (g, w) in enumerate(zip(got[name]['calls'], want[name]['calls'])):
            assert digest(g) == w, (name, i, g)


if __name__ == '__main__':
    import sys
    mp = pytest.MonkeyPatch()
    rec = json.loads(json.dumps({arm: record(mp, arm) for arm in ('f32', 'bf16')}))
    mp.undo()
    if '--full' in sys.argv:
        for arm in rec:
            for name, v in rec[arm].items():
                for i, c in enumerate(v['calls']):
                    print(arm, name, i, json.dumps(c, separators=(',', ':')))
    else:                                                                      # one sequence per line
        one = lambda v: json.dumps(dict(v, calls=[digest(c) for c in v['calls']]), separators=(',', ':'))
        print('{' + ',\n'.join('"%s":{\n%s}' % (arm, ',\n'.join('"%s":%s' % (n, one(v)) for n, v in rec[arm].items())) for arm in rec) + '}')
