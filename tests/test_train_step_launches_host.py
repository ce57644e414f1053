"""CPU: the launch sequences of ``MIGTTrainer``.  Every ``ops`` / ``train_ops`` function the trainer calls, and
``MIGT._gemm``, is replaced by the recorder of tests/test_context_cache_launches_host.py: it returns correctly shaped CPU tensors and
writes down the function's name and every argument (tensors as dtype, shape, stride, offset and the number of their storage).
``torch.cuda.current_stream`` / ``Stream`` / ``stream`` are fakes that append 'new_stream', 'wait_stream', 'enter' and 'exit' events to
the same sequence, ``Tensor.record_stream`` and ``Tensor.zero_`` are recorded too: which stream a launch goes to, who waits for whom and
which gradient ranges are zero-filled are part of the record.  Construction (``_bind`` + ``repack``), a first and a second step on six
shapes that between them make every ``StepPlan`` field true and false, one step with each switch changed, ``test_step`` and a step
without reduction and update must equal ``tests/golden/train_step_launches.json``, recorded before ``train_step`` became a sequence of
phases.  The fixture keeps every call as 'name:digest'; a call that differs is reported with its live arguments.  No device is touched.

``python tests/test_train_step_launches_host.py`` prints the fixture of the code as it stands, ``... --full`` every call with its
arguments, one per line, for a diff between two checkouts."""
import contextlib
import json
import os

import pytest
import torch

from test_context_cache_launches_host import Recorder, digest, host_records

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_step_launches.json')
D, H, NE, NL = 256, 4, 256, 2            # the smallest model at which every plan field can be true (256-wide tiles, 64-wide heads)

#        name        precision NS B  S  L   config / trainer attributes
CASES = {'bf16_tail': ('bf16', 2, 2, 2, 64, {}, {}),                                   # tail, every fast path but drop16
         'bf16_drop': ('bf16', 2, 2, 2, 64, dict(dropout=0.1), dict(scene_offset=3)),  # ... and drop16
         'bf16_full': ('bf16', 2, 1, 3, 64, {}, {}),                                   # Mx would be 192: no tail
         'bf16_attn32': ('bf16', 3, 1, 3, 64, {}, {}),                                 # tail, M = 576: no bf16 operands
         'bf16_L16': ('bf16', 2, 2, 2, 16, {}, {}),                                    # exact-f32 attention on the bf16 arm
         'f32_tail': ('f32', 3, 1, 2, 64, {}, {})}                                     # native / split arm with the tail


class StepRecorder(Recorder):
    """floats to 12 digits (a learning rate's last bit is libm's), small int64 tensors (the no-decay ranges) with their values, no
    keyword that is None (every keyword the trainer passes defaults to None: passing it or leaving it out is the same launch)"""

    def wrap(self, name, result=lambda *a, **k: None):
        def fn(*a, **k):
            kw = {n: self.arg(k[n]) for n in sorted(k) if k[n] is not None}
            self.calls.append([name] + [self.arg(x) for x in a] + [kw] * bool(kw))
            return result(*a, **k)
        return fn

    def arg(self, x):
        if isinstance(x, float):
            return float('%.12g' % x)
        if isinstance(x, torch.device):
            return str(x)
        r = super().arg(x)
        if isinstance(x, torch.Tensor) and x.dtype == torch.int64 and x.numel() <= 64:
            r += ('=%s' % x.reshape(-1).tolist()).replace(' ', '')
        return r


class _Stream:
    def __init__(self, rec, name):
        self.rec, self.name = rec, name

    def wait_stream(self, other):
        self.rec.calls.append(['wait_stream', self.name, other.name])


class _Streams:
    """torch.cuda's stream calls on one recorder: streams are named in the order they are created"""

    def __init__(self, rec):
        self.rec, self.stack, self.n = rec, [_Stream(rec, 'main')], 0

    def current_stream(self, device=None):
        return self.stack[-1]

    def Stream(self, device=None):
        self.n += 1
        self.rec.calls.append(['new_stream', 's%d' % self.n])
        return _Stream(self.rec, 's%d' % self.n)

    @contextlib.contextmanager
    def stream(self, s):
        self.rec.calls.append(['enter', s.name])
        self.stack.append(s)
        try:
            yield
        finally:
            self.stack.pop()
            self.rec.calls.append(['exit', s.name])


def _pf(K, N, taps=1):
    return (K + 31) // 32 * 32 * ((N + 31) // 32 * 32) * taps


def _f(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def _b16(on):
    return torch.bfloat16 if on else torch.float32


def _patch(monkeypatch, rec):
    from viewformer_amd import ops
    from viewformer_amd import train_ops as T
    nothing = lambda *a, **k: None                                                      # noqa: E731
    ops_stubs = dict(
        igemm=nothing, gemm_tn_bf16=nothing, gemm_bf16_splitk=nothing, gemm_x6_splitk=nothing,
        pack=lambda src, K, N, taps, sk, sn, st, batch=1, src_bstride=0, out=None: out if out is not None else _f(batch * _pf(K, N, taps)),
        pack_dense_kn_bf16=lambda w: _f(w.shape[0] * w.shape[1], dtype=torch.bfloat16),
        pack_dense_nk_bf16=lambda w, n_rows=None: _f(w.shape[0] * w.shape[1], dtype=torch.bfloat16),
        pack_dense_kn_x6=lambda w: _f(3 * w.shape[0] * w.shape[1], dtype=torch.bfloat16),
        pack_dense_nk_x6=lambda w, n_rows=None: _f(3 * w.shape[0] * w.shape[1], dtype=torch.bfloat16),
        pack_dense_kn_x3h=lambda w: _f(2 * w.shape[0] * w.shape[1], dtype=torch.float16),
        pack_bf16_multi=lambda items: rec.wrap('_pack16'),
        dense_small_k=lambda x, W, b, rows, K, n, gelu: _f(rows, n),
        embed_sum=lambda ids, wte, wpe, add, BS, L, d, vocab: _f(BS * L, d),
        layernorm=lambda x, g, b, rows, d, out_bf16=False: _f(rows, d, dtype=_b16(out_bf16)),
        argmax_rows=lambda x, rows, n: torch.zeros(rows, dtype=torch.int64))
    t_stubs = dict(
        attn_bwd=nothing, attn_bwd_bf16=nothing, dense_small_k_bwd=nothing, adamw_=nothing, adamw_flat_=nothing, adamw_flat_pack_=nothing,
        dropout_add=lambda x, rate, seed, site, res=None, out=None, cols=None, row0=0: out if out is not None else torch.zeros_like(x),
        colsum=lambda x, out, M, N, ld=None, accumulate=False: out,
        transpose=lambda src, rows, cols, ld_src=None, batch=1, bs_src=0, out=None, ld_dst=None:
            out if out is not None else _f(batch, cols, rows if ld_dst is None else ld_dst),
        layernorm_bwd=lambda dy, x, gamma, dgamma, dbeta, rows, d, eps=1e-5, accumulate=True, res=None, also_bf16=False, drop=(0.0, 0, 0):
            (_f(*x.shape), _f(*x.shape, dtype=torch.bfloat16)) if also_bf16 else _f(*x.shape),
        gelu=lambda u, out_bf16=False: _f(*u.shape, dtype=_b16(out_bf16)),
        gelu_bwd=lambda u, df, out_bf16=False: _f(*u.shape, dtype=_b16(out_bf16)),
        attn_fwd_lse=lambda q, k, v, out, B, H_, T_, *a, **kw: _f(B, H_, T_),
        attn_fwd_lse_bf16=lambda q, k, v, out, B, H_, T_, *a, **kw: _f(B, H_, T_),
        softmax_mask_=lambda s, *a: s,
        softmax_mask_bwd_=lambda p, dp, *a: dp,
        softmax_ce=lambda logits, tgt, w, rows, V, ls=0.0: (_f(rows), _f(rows, V)),
        pose_mse=lambda raw, gt, w, rows, L, pm, w_ori=None, xyz_div=None: (_f(rows), _f(rows), _f(rows, 7)),
        embed_bwd=lambda dh, ids, dwte, dwpe, BS, L, d, vocab: _f(BS, d),
        dense_small_n=lambda x, W, b, rows, K, N: _f(rows, N),
        dense_small_n_wgrad=lambda x, dy, dW, rows, K, N, accumulate=True: dW,
        adamw_pack_table=lambda flat, items, nodecay=None: (torch.zeros(40 * len(items), dtype=torch.uint8), len(items)),
        clip_scratch=lambda device: _f(8),
        clip_by_norm_=lambda x, clip, scratch: x)
    for mod, stubs in ((ops, ops_stubs), (T, t_stubs)):
        for name, fn in stubs.items():
            monkeypatch.setattr(mod, name, rec.wrap(name, fn))
    monkeypatch.setattr(ops, 'packed_floats', _pf)                                      # (a size, not a launch)
    streams = _Streams(rec)
    for name in ('current_stream', 'Stream', 'stream'):
        monkeypatch.setattr(torch.cuda, name, getattr(streams, name))
    monkeypatch.setattr(torch.Tensor, 'record_stream', lambda t, s: rec.calls.append(['record_stream', rec.arg(t), s.name]), raising=False)
    zero_ = torch.Tensor.zero_
    monkeypatch.setattr(torch.Tensor, 'zero_', lambda t: (rec.calls.append(['zero_', rec.arg(t)]), zero_(t))[1])


def _trainer(rec, precision, NS, L, cfg_kw, attrs):
    """a host model with the generated weights' shapes, every launch a recorder, and its trainer"""
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.train import MIGTTrainer
    from viewformer_amd.weights import make_migt_weights
    cfg = MIGTConfig(**dict(dict(n_embeddings=NE, n_head=H, d_model=D, n_layer=NL, token_image_size=int(L ** 0.5), sequence_size=4, n_loss_skip=1,
                                 dropout=0.0, localization_weight='1' if NS == 3 else '0'), **cfg_kw))
    m = MIGT(cfg, precision=precision).load_state_dict(make_migt_weights(cfg))
    m.device = torch.device('cpu')
    host_records(m, {k[:-7]: m._sd_host[k].shape for k in m.expected_keys() if k.endswith('.weight') and k != 'wte.weight'}, tensors=False)
    for k in m.expected_keys():
        if k.endswith('.gamma'):
            m._ln[k[:-6]] = None
    m._gemm = rec.wrap('_gemm', lambda x, name, M, epilogue=None, res=None, out_bf16=False: _f(M, m._dense[name].n, dtype=_b16(out_bf16)))
    tr = MIGTTrainer(m)
    for k, v in attrs.items():
        setattr(tr, k, v)
    return tr


def _batch(B, S, L):
    t = int(L ** 0.5)
    poses = torch.zeros(B, S, 7)
    poses[..., 3] = 1.0
    return poses, (torch.arange(B * S * L) % NE).view(B, S, t, t)


def record(monkeypatch):
    from viewformer_amd.train import MIGTTrainer, PLAN_SWITCHES
    rec = StepRecorder()
    _patch(monkeypatch, rec)
    out = {}

    def seq(name, fn):
        rec.reset()
        res = fn()
        out[name] = rec.calls
        return res

    for name, (precision, NS, B, S, L, cfg_kw, attrs) in CASES.items():
        tr = seq(name + '/construct', lambda: _trainer(rec, precision, NS, L, cfg_kw, attrs))
        batch = _batch(B, S, L)
        seq(name + '/step1', lambda: tr.train_step(*batch))
        seq(name + '/step2', lambda: tr.train_step(*batch))
        out[name + '/plan'] = [json.dumps(tr.last_plan._asdict(), sort_keys=True)]

    def variant(name, case='bf16_tail', NS=None, cfg_kw=None, late=None, step=None, **switches):
        """construction and one step with class-level ``switches`` (as the A/B tools set them); ``late``: set on the built trainer"""
        precision, ns, B, S, L, kw, attrs = CASES[case]
        with monkeypatch.context() as mp:
            for k, v in switches.items():
                assert hasattr(MIGTTrainer, k), k
                mp.setattr(MIGTTrainer, k, v)

            def run():
                tr = _trainer(rec, precision, NS or ns, L, dict(kw, **(cfg_kw or {})), dict(attrs, **(late or {})))
                return (step or (lambda tr, batch: tr.train_step(*batch)))(tr, _batch(B, S, L))
            seq(name, run)

    for k in PLAN_SWITCHES:
        variant('switch/' + k, **{k: 'f32' if k == 'attention_arith' else not getattr(MIGTTrainer, k)})
        variant('switch_drop/' + k, case='bf16_drop', **{k: 'f32' if k == 'attention_arith' else not getattr(MIGTTrainer, k)})
    for k, v in (('overlap_weight_gradients', False), ('lazy_gradient_zero', False), ('early_optimizer', True), ('fused_optimizer', False),
                 ('fused_optimizer_repack', False), ('bf16_lm_head', False), ('one_launch_repack', False)):
        variant('switch/%s=%s' % (k, v), **{k: v})
    variant('switch/early_optimizer_two_steps', early_optimizer=True, step=lambda tr, b: (tr.train_step(*b), tr.train_step(*b)))
    variant('switch/fused_optimizer_repack_two_steps', fused_optimizer_repack=False, step=lambda tr, b: (tr.train_step(*b), tr.train_step(*b)))
    variant('switch/bf16_lm_head_late', late=dict(bf16_lm_head=False), step=lambda tr, b: (tr.train_step(*b), tr.train_step(*b)))
    variant('switch/small_n_pose_head=False', NS=3, small_n_pose_head=False)
    variant('switch/small_n_pose_head=True', NS=3)
    variant('switch/attention_backward=dense', case='f32_tail', attention_backward='dense')
    variant('config/gradient_clip_val', cfg_kw=dict(gradient_clip_val=1.0))
    variant('config/gradient_clip_val_early', cfg_kw=dict(gradient_clip_val=1.0), early_optimizer=True)
    variant('config/weight_decay=0', cfg_kw=dict(weight_decay=0.0))
    variant('config/use_dynamic_pose_loss', NS=3, cfg_kw=dict(use_dynamic_pose_loss=True))
    variant('config/random_pose_multiplier', NS=3, cfg_kw=dict(random_pose_multiplier=3.0))
    variant('config/random_pose_multiplier_drop', case='bf16_drop', NS=3, cfg_kw=dict(random_pose_multiplier=3.0))
    for case in ('bf16_tail', 'bf16_attn32', 'f32_tail'):
        variant('test_step/' + case, case=case, step=lambda tr, b: tr.test_step(*b))
        variant('no_reduce_no_update/' + case, case=case,
                step=lambda tr, b: (tr.train_step(*b, reduce_gradients=False, apply_update=False), tr.apply_gradients()))
    return out


def test_the_trainer_issues_the_recorded_launches(monkeypatch):
    got = json.loads(json.dumps(record(monkeypatch)))
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert sorted(got) == sorted(want)
    for name in want:
        if name.endswith('/plan'):
            assert got[name] == want[name], name
            continue
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert digest(g) == w, (name, i, g)
        assert len(got[name]) == len(want[name]), name


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    mp = pytest.MonkeyPatch()
    rec = json.loads(json.dumps(record(mp)))
    mp.undo()
    if '--full' in sys.argv:
        for name, calls in rec.items():
            for i, c in enumerate(calls):
                print(name, i, json.dumps(c, separators=(',', ':')))
    else:                                                                      # one sequence per line
        one = lambda n, v: json.dumps(v if n.endswith('/plan') else [digest(c) for c in v], separators=(',', ':'))      # noqa: E731
        print('{' + ',\n'.join('"%s":%s' % (n, one(n, v)) for n, v in rec.items()) + '}')
