"""CPU: which packing and which keywords the transformer's host code hands to ``ops.igemm``.  Every launching ``ops`` /
``train_ops`` function ``MIGT`` and ``MIGTTrainer`` call around a dense layer is replaced by the recorder of
tests/test_codec_launches_host.py: it returns correctly shaped CPU tensors and writes down the function's name and every argument,
bound to the real function's signature with its defaults filled in.  The pure-Python ``*_supported`` mirrors stay real, and so do
``MIGT._upload``, ``_gemm`` and ``_dense_launch``: the models here are built by the code under test, not by hand.

Per model case — (precision, dense_arith) in f32/f32, f32/x6, f32/x3h, bf16/x3h at d_model 96 (k % 32 == 0 but not % 64: every layer and
the head native) and 128 (the wide layers and the head on the fast arm; the pose classifier's 7-column c_proj native,
pose_embedding.c_fc unpacked), with 64 codes, and once more on the bf16 arm with the 128 codes the fused LM-head kernels need — ``_upload`` (which packer on which layer, in order), ``_gemm`` on every packed layer with fp32 rows (and
with bf16 rows and a bf16 result on the bf16 arm), ``_pose_embed`` (the one unpacked layer), ``_lm``, ``_lm_argmax``, ``_lm_score`` fused
and not, ``_linear_dx`` of the head and of a layer twice (the second call packs nothing), ``_pose_embed_bwd`` twice, and ``_linear_dx``
after a second ``load_state_dict`` (it packs again: the cache belongs to the weights).

For the trainer, on the d_model 256 model of tests/test_train_step_launches_host.py and the bf16, x6 and x3h arms: construction, then
``_linear``, ``_proj_dropout`` (no dropout, unfused, fused), ``_weight_gradient`` and ``_linear_dx`` at 128, 64 and 32 rows — both sides
of M % 128 and M % 64 — a second ``repack``, and the model's own ``_lm`` afterwards (the native launch, whatever the trainer packed).
A refusal is recorded with its text.  All of it must equal ``tests/golden/migt_dense_launches.json``, recorded before the packings
moved into one record per layer; a call that differs is reported with its live arguments.  No device is touched.

``python tests/test_migt_dense_launches_host.py`` prints the fixture of the code as it stands, ``... --full`` every call with its
arguments, one per line, for a diff between two checkouts."""
import json
import os

import pytest
import torch

from test_codec_launches_host import CodecRecorder
from test_context_cache_launches_host import digest
from test_train_step_launches_host import _Streams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'migt_dense_launches.json')
ARMS = (('f32', 'f32'), ('f32', 'x6'), ('f32', 'x3h'), ('bf16', 'x3h'))                  # (precision, dense_arith)
NE, L = 64, 64
TD, TH, TNE, TNL = 256, 4, 256, 2                                                        # the trainer's model
ROWS = (128, 64, 32)
b16, f16 = torch.bfloat16, torch.float16


def _e(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def _pf(K, N, taps=1):
    return (K + 31) // 32 * 32 * ((N + 31) // 32 * 32) * taps


def _nk(w, n_rows):
    return (n_rows or w.shape[0]) * w.shape[1]


def _score(rows, target, want):
    return {k: _e(rows, dtype=torch.int64 if k == 'idx' else torch.float32) for k in want}


def _patch(monkeypatch, rec):
    from viewformer_amd import ops
    from viewformer_amd import train_ops as T
    nothing = lambda *a, **k: None                                                      # noqa: E731
    ops_stubs = dict(
        igemm=nothing, gemm_tn_bf16=nothing, gemm_bf16_splitk=nothing, gemm_x6_splitk=nothing,
        pack=lambda src, K, N, taps, sk, sn, st, batch=1, src_bstride=0, out=None: out if out is not None else _e(batch * _pf(K, N, taps)),
        pack_dense_kn=lambda w: _e(_pf(*w.shape)),
        pack_dense_nk=lambda w, n_rows=None: _e(_pf(w.shape[1], n_rows or w.shape[0])),
        pack_dense_kn_bf16=lambda w: _e(w.numel(), dtype=b16),
        pack_dense_nk_bf16=lambda w, n_rows=None: _e(_nk(w, n_rows), dtype=b16),
        pack_dense_kn_x6=lambda w: _e(3 * w.numel(), dtype=b16),
        pack_dense_nk_x6=lambda w, n_rows=None: _e(3 * _nk(w, n_rows), dtype=b16),
        pack_dense_kn_x3h=lambda w: _e(2 * w.numel() + 2, dtype=f16),
        pack_dense_nk_x3h=lambda w, n_rows=None: _e(2 * _nk(w, n_rows) + 2, dtype=f16),
        pack_bf16_multi=lambda items: rec.wrap('_pack16', lambda first=0, count=None: None),
        dense_small_k=lambda x, W, b, rows, K, N, gelu: _e(rows, N),
        lmhead_argmax_bf16=lambda h, w, M, K, N, want_max=False: torch.zeros(M, dtype=torch.int64),
        lmhead_score_bf16=lambda h, w, M, K, N, target=None, want=ops.SCORE_OUTPUTS: _score(M, target, want),
        logits_score=lambda lg, rows, N, target=None, want=ops.SCORE_OUTPUTS, ld=None: _score(rows, target, want))
    t_stubs = dict(
        gelu_bwd=lambda u, df, out_bf16=False: _e(*u.shape, dtype=b16 if out_bf16 else torch.float32),
        transpose=lambda src, rows, cols, ld_src=None, batch=1, bs_src=0, out=None, ld_dst=None:
            out if out is not None else _e(batch, cols, rows if ld_dst is None else ld_dst),
        dense_small_n=lambda x, W, b, rows, K, N: _e(rows, N),
        colsum=lambda x, out, M, N, ld=None, accumulate=False: out,
        dropout_add=lambda x, rate, seed, site, res=None, out=None, cols=None, row0=0: out if out is not None else torch.zeros_like(x),
        adamw_pack_table=lambda flat, items, nodecay=None: (torch.zeros(40 * len(items), dtype=torch.uint8), len(items)))
    for mod, stubs in ((ops, ops_stubs), (T, t_stubs)):
        for name, fn in stubs.items():
            monkeypatch.setattr(mod, name, rec.wrap(name, getattr(mod, name), fn))
    monkeypatch.setattr(ops, 'packed_floats', _pf)                                      # (a size, not a launch)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda device=None: None)
    streams = _Streams(rec)
    for name in ('current_stream', 'Stream', 'stream'):
        monkeypatch.setattr(torch.cuda, name, getattr(streams, name))
    monkeypatch.setattr(torch.Tensor, 'record_stream', lambda t, s: rec.calls.append(['record_stream', rec.arg(t), s.name]), raising=False)


def _model(cfg, precision, arith):
    """a model of the generated weights' shapes on the CPU: the real ``_upload`` over the recorded packers"""
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    m = MIGT(cfg, precision=precision, dense_arith=arith)
    m.device = torch.device('cpu')
    return m, make_migt_weights(cfg)


def _attempt(rec, fn):
    try:
        return fn()
    except RuntimeError as e:
        rec.calls.append(['raises', type(e).__name__, str(e)])


def _record_model(rec, seq, name, precision, arith, d, NE=NE):
    from viewformer_amd import ops
    from viewformer_amd.config import MIGTConfig
    cfg = MIGTConfig(n_embeddings=NE, n_head=2, d_model=d, n_layer=1, token_image_size=8, sequence_size=4)
    m, sd = _model(cfg, precision, arith)
    seq(name + '/upload', lambda: m.load_state_dict(sd))
    M = 64
    layers = [n for n in m._dense if n != 'pose_embedding.c_fc']                          # (unpacked: dense_small_k reads the raw weight, _pose_embed)

    def gemms():
        for n in layers:
            dn = m._dense[n]
            y = m._gemm(_e(M, dn.k), n, M)
            assert tuple(y.shape) == (M, dn.n) and y.dtype == torch.float32
            m._gemm(_e(M, dn.k), n, M, epilogue=ops.EPI_GELU, res=_e(M, dn.n))
    seq(name + '/gemm', gemms)
    if precision == 'bf16' and d % 64 == 0:
        wide = [n for n in layers if m._dense[n].n >= 64]
        seq(name + '/gemm_bf16_rows', lambda: [m._gemm(_e(M, m._dense[n].k, dtype=b16), n, M, out_bf16=True) for n in wide])
    seq(name + '/pose_embed', lambda: m._pose_embed(_e(2, 3, 7)))
    seq(name + '/lm', lambda: m._lm(_e(M, d), M, _e(M, NE)))
    seq(name + '/lm_argmax', lambda: rec.calls.append(['returns', m._lm_argmax(_e(M, d), M) is not None]))
    for fused in (False, True):
        st = seq(name + '/lm_score/fused=%s' % fused, lambda: m._lm_score(_e(M, d), M, torch.zeros(M, dtype=torch.int32), fused=fused))
        assert sorted(st) == sorted(ops.SCORE_OUTPUTS)
    for n in ('wte', 'h.0.mlp.c_fc', 'pose_criterion.pose_classifier.c_proj'):
        nn = NE if n == 'wte' else m._dense[n].n
        for i in (1, 2):
            seq(name + '/linear_dx/%s/%d' % (n, i), lambda: m._linear_dx(n, _e(M, nn), M))
    for i in (1, 2):
        g = seq(name + '/pose_embed_bwd/%d' % i, lambda: m._pose_embed_bwd(_e(2, 3, 7), _e(6, d)))
        assert tuple(g.shape) == (2, 3, 7)
    seq(name + '/upload_again', lambda: m.load_state_dict(sd))
    for n in ('wte', 'h.0.mlp.c_fc'):
        seq(name + '/linear_dx_after_upload/' + n, lambda: m._linear_dx(n, _e(M, NE if n == 'wte' else m._dense[n].n), M))
    seq(name + '/pose_embed_bwd_after_upload', lambda: m._pose_embed_bwd(_e(2, 3, 7), _e(6, d)))


def _record_trainer(rec, seq, name, precision, arith):
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.train import MIGTTrainer
    cfg = MIGTConfig(n_embeddings=TNE, n_head=TH, d_model=TD, n_layer=TNL, token_image_size=8, sequence_size=4, n_loss_skip=1, dropout=0.1,
                     localization_weight='1')
    m, sd = _model(cfg, precision, arith)

    def construct():
        m.load_state_dict(sd)
        return MIGTTrainer(m)
    tr = seq(name + '/construct', construct)
    tr._unset = set()
    fwd = [n for n in m._dense if n.startswith('h.0.') or n.startswith('pose_c') or n == 'pose_embedding.c_proj']
    bwd = fwd + ['pose_embedding.c_fc']
    lp = precision == 'bf16'
    for M in ROWS:
        tag = '%s/M=%d/' % (name, M)
        seq(tag + 'linear', lambda: [tr._linear(_e(M, m._dense[n].k), n, M, res=_e(M, m._dense[n].n)) for n in fwd])

        def proj():
            for n in ('h.0.attn.c_proj', 'h.0.mlp.c_proj'):
                dn = m._dense[n]
                res = _e(M, dn.n)
                for dt in (torch.float32,) + (b16,) * lp:
                    tr._proj_dropout(_e(M, dn.k, dtype=dt), n, M, res, (0.0, 0, 0, 0))
                    tr._proj_dropout(_e(M, dn.k, dtype=dt), n, M, res, (0.1, 5, 17, 4), fused=False)
                    tr._proj_dropout(_e(M, dn.k, dtype=dt), n, M, res, (0.1, 5, 17, 4), fused=True)
        seq(tag + 'proj_dropout', proj)

        def wgrad():
            for n in bwd:
                dn = m._dense[n]
                for follows in (True, False):
                    tr._weight_gradient(n, _e(M, dn.k), _e(M, dn.n), M, follows)
                    tr._join_side()
                if lp:
                    for follows in (True, False):
                        _attempt(rec, lambda: tr._weight_gradient(n, _e(M, dn.k, dtype=b16), _e(M, dn.n, dtype=b16), M, follows))
                        tr._join_side()
                    tr._unset = {n}                                               # (the layer's first writer of a step stores)
                    tr._weight_gradient(n, _e(M, dn.k, dtype=b16), _e(M, dn.n), M, True)
                    tr._join_side()
        seq(tag + 'weight_gradient', wgrad)

        def dx():
            for n in bwd:
                dn = m._dense[n]
                tr._linear_dx(n, _e(M, dn.n), M)
                tr._linear_dx(n, _e(M, dn.n), M, res=_e(M, dn.k))
                if lp:
                    u = _e(M, dn.k, dtype=b16)
                    _attempt(rec, lambda: tr._linear_dx(n, _e(M, dn.n, dtype=b16), M, dx_bf16=True))
                    _attempt(rec, lambda: tr._linear_dx(n, _e(M, dn.n), M, res=_e(M, dn.k), dx_bf16=True))
                    _attempt(rec, lambda: tr._linear_dx(n, _e(M, dn.n, dtype=b16), M, dx_bf16=True, gelu_bwd_u=u, u_is_derivative=True))
                    _attempt(rec, lambda: tr._linear_dx(n, _e(M, dn.n, dtype=b16), M, dx_bf16=True, gelu_bwd_u=_e(M, dn.k)))
                    _attempt(rec, lambda: tr._linear_dx(n, _e(M, dn.n), M, gelu_bwd_u=u))
        seq(tag + 'linear_dx', dx)
    seq(name + '/repack', tr.repack)
    seq(name + '/repack_early_layers_done', lambda: tr.repack(early_layers_done=True))
    seq(name + '/model_lm_after_repack', lambda: m._lm(_e(64, TD), 64, _e(64, TNE)))
    seq(name + '/model_lm_argmax_after_repack', lambda: rec.calls.append(['returns', m._lm_argmax(_e(64, TD), 64) is not None]))


def record(monkeypatch):
    rec = CodecRecorder()
    _patch(monkeypatch, rec)
    out = {}

    def seq(name, fn):
        rec.reset()
        res = fn()
        out[name] = rec.calls
        return res

    for precision, arith in ARMS:
        for d in (96, 128):
            _record_model(rec, seq, 'model/%s/%s/d=%d' % (precision, arith, d), precision, arith, d)
            rec.keep.clear()
    _record_model(rec, seq, 'model/bf16/x3h/d=128/ne=128', 'bf16', 'x3h', 128, NE=128)      # ... and a head the fused arg-max and score take
    rec.keep.clear()
    for precision, arith in (('bf16', 'x3h'), ('f32', 'x6'), ('f32', 'x3h')):
        _record_trainer(rec, seq, 'trainer/%s/%s' % (precision, arith), precision, arith)
        rec.keep.clear()
    return out


def test_the_second_transposed_use_packs_nothing(monkeypatch):
    """the fixture's own claims about the transposed caches, stated: a second ``_linear_dx`` / ``_pose_embed_bwd`` issues no packer, the
    first after new weights issues one again"""
    got = record(monkeypatch)
    packs = lambda calls: [c[0] for c in calls if c[0].startswith('pack') or c[0] == 'transpose']      # noqa: E731
    for name, calls in got.items():
        if '/linear_dx/' in name and name.startswith('model/'):
            assert len(packs(calls)) == (1 if name.endswith('/1') else 0), name
        if '/linear_dx_after_upload/' in name:
            assert len(packs(calls)) == 1, name
        if name.endswith('/pose_embed_bwd/1') or name.endswith('/pose_embed_bwd_after_upload'):
            assert packs(calls) == ['pack', 'transpose'], name
        if name.endswith('/pose_embed_bwd/2'):
            assert packs(calls) == [], name
        if name.endswith('/model_lm_after_repack'):
            (call,) = calls
            assert call[0] == 'igemm' and not (call[1]['bf16'] or call[1]['x6'] or call[1]['x3h']) and call[1]['w_packed'].startswith('float32'), name


def test_the_transformer_issues_the_recorded_launches(monkeypatch):
    got = json.loads(json.dumps(record(monkeypatch)))
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert sorted(got) == sorted(want)
    for name in want:
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
        print('{' + ',\n'.join('"%s":%s' % (n, json.dumps([digest(c) for c in v], separators=(',', ':'))) for n, v in rec.items()) + '}')
