"""CPU: the launch sequences of the VQGAN codec's host code.  Every ``ops`` function ``VQGAN`` calls is replaced by the
recorder of tests/test_context_cache_launches_host.py: it returns correctly shaped CPU tensors and writes down the function's name and
every argument, bound to the real function's signature with its defaults filled in (a keyword left out and a keyword passed at its
default are the same launch).  The pure-Python ``*_supported`` mirrors of ``ops`` stay real, so the rules that pick a layer's arithmetic
run as they do on the device.  Per case three sequences: ``_upload`` (which packer on which layer, in order), ``encode`` and
``decode_code``.  The cases take, and do not take, every branch of the choice: the three arithmetics with both decoder precisions,
the four ``decoder_act16`` values, channel counts at which the activation stream may not switch to bf16, every switch, the tiny
configuration of tests/golden/vqgan_tiny.npz, and 64x64 images (8x8 bottom level, a bf16 halo rule that fails below 16 wide).  The
refusals of a bf16 activation are recorded with their texts.  ``VQGANTrainer._conv_launch`` and ``LPIPS._conv`` are recorded on the
smallest shapes on each side of ``conv3_x6_supported`` and ``conv3_small_cout_supported``.  All of it must equal
``tests/golden/codec_launches.json``, recorded before the choice of arithmetic moved into one chooser; a call that differs is reported
with its live arguments.  No device is touched.

``python tests/test_codec_launches_host.py`` prints the fixture of the code as it stands, ``... --full`` every call with its
arguments, one per line, for a diff between two checkouts."""
import inspect
import json
import os

import pytest
import torch

from test_context_cache_launches_host import Recorder, digest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'codec_launches.json')
TINY_VQ = dict(ch=32, ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[16], image_size=32, z_channels=32, embed_dim=32, n_embed=64)

#        name                  config       constructor                                          attributes / environment      images, side
CASES = {}
for _a in ('f32', 'x6', 'x3h'):
    for _p in ('f32', 'bf16'):
        CASES[f'default/{_a}/{_p}'] = ({}, dict(conv_arith=_a, decoder_precision=_p), {}, 1, 128)
    CASES[f'tiny/{_a}'] = (TINY_VQ, dict(conv_arith=_a), {}, 1, 32)
for _r in (0, 32, 64):                                                                  # 128 is the default above
    CASES[f'act16={_r}'] = ({}, dict(conv_arith='x3h', decoder_precision='bf16'), dict(decoder_act16=_r), 1, 128)
for _c in (64, 96):                                                                     # the stream may not switch to bf16
    CASES[f'ch={_c}'] = (dict(ch=_c), dict(conv_arith='x3h', decoder_precision='bf16'), {}, 1, 128)
CASES.update({
    'fuse_gn_stats=False': ({}, dict(conv_arith='x3h'), dict(fuse_gn_stats=False), 1, 128),
    'fuse_gn_stats=False/bf16': ({}, dict(conv_arith='x3h', decoder_precision='bf16'), dict(fuse_gn_stats=False), 1, 128),
    'fused_attention=False': ({}, dict(conv_arith='x3h'), dict(fused_attention=False), 1, 128),
    'VF_VQ_DENSE_X3H=0': ({}, dict(conv_arith='x3h'), dict(VF_VQ_DENSE_X3H='0'), 1, 128),
    'VF_VQ_DENSE_X3H=0/bf16': ({}, dict(conv_arith='x3h', decoder_precision='bf16'), dict(VF_VQ_DENSE_X3H='0'), 1, 128),
    'lookup=exact': ({}, dict(conv_arith='x3h', lookup='exact'), {}, 1, 128),
    'three_64x64/x3h/bf16': ({}, dict(conv_arith='x3h', decoder_precision='bf16'), {}, 3, 64),
    'three_64x64/x6/f32': ({}, dict(conv_arith='x6'), {}, 3, 64),
    'three_64x64/x3h/act16=32': ({}, dict(conv_arith='x3h', decoder_precision='bf16'), dict(decoder_act16=32), 3, 64)})


class CodecRecorder(Recorder):
    """every call as {parameter name: argument} of the real function's signature, defaults included"""

    def wrap(self, name, real, result=lambda *a, **k: None):
        sig = inspect.signature(real)

        def fn(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            self.calls.append([name, {n: self.arg(v) for n, v in b.arguments.items()}])
            return result(*a, **k)
        return fn

    def arg(self, x):
        return str(x) if isinstance(x, torch.device) else super().arg(x)


def _e(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype)


def _pf(K, N, taps=1):
    return (K + 31) // 32 * 32 * ((N + 31) // 32 * 32) * taps


def _slots(Hout, Wout):
    """one slot per 8 x 16 output tile where the halo kernels tile the output (the shape only sizes a buffer here)"""
    return (Hout // 8) * (Wout // 16) if Hout % 8 == 0 and Wout % 16 == 0 else 1 if (Hout, Wout) == (8, 8) else 0


def _patch(monkeypatch, rec):
    from viewformer_amd import ops
    b16, f16 = torch.bfloat16, torch.float16
    stubs = dict(
        pack=lambda src, K, N, taps, sk, sn, st, batch=1, src_bstride=0, out=None: out if out is not None else _e(batch * _pf(K, N, taps)),
        pack_conv_oihw=lambda w: _e(_pf(w.shape[1], w.shape[0], w.shape[2] * w.shape[3])),
        pack_dense_kn=lambda w: _e(_pf(*w.shape)),
        pack_dense_nk=lambda w, n_rows=None: _e(_pf(w.shape[1], n_rows or w.shape[0])),
        pack_dense_kn_bf16=lambda w: _e(w.numel(), dtype=b16),
        pack_dense_nk_bf16=lambda w, n_rows=None: _e(w.numel(), dtype=b16),
        pack_dense_kn_x6=lambda w: _e(3 * w.numel(), dtype=b16),
        pack_dense_nk_x6=lambda w, n_rows=None: _e(3 * w.numel(), dtype=b16),
        pack_dense_kn_x3h=lambda w: _e(2 * w.numel() + 2, dtype=f16),
        pack_dense_nk_x3h=lambda w, n_rows=None: _e(2 * w.numel() + 2, dtype=f16),
        pack_conv3_bf16=lambda w: _e(w.numel(), dtype=b16),
        pack_conv3_x6=lambda w: _e(3 * w.numel(), dtype=b16),
        pack_conv3_x3h=lambda w: _e(2 * w.numel() + 2, dtype=f16),
        pack_conv_in_x3h=lambda w: _e(2 * 32 * w.shape[0] + 2, dtype=f16),
        vq_pack_codebook=lambda E: (_e(E.numel()), _e(E.shape[1])),
        vq_filter_pack=lambda E: _e(16, dtype=torch.uint8),
        vq_filter_supported=lambda D, Kc: D == 256 and Kc % 32 == 0 and Kc <= 1024,
        igemm=lambda *a, **k: None,
        conv_in=lambda img, w, bias, n, H, W, Cout, out=None, wp3h=None, gn_part=None: out if out is not None else _e(n, H, W, Cout),
        conv3_small_cout=lambda x, w, bias, n, H, W, Cin, Cout, pro=None, pro_swish=True, out=None:
            out if out is not None else _e(n * H * W, Cout),
        groupnorm_stats=lambda x, gamma, n, HW, C, groups=32, eps=1e-6: (_e(n, C), _e(n, C)),
        groupnorm_finalize=lambda part, gamma, n, HW, C, groups=32, eps=1e-6: (_e(n, C), _e(n, C)),
        groupnorm_apply=lambda x, mean_c, scale_c, beta, n, HW, C, swish, out=None: out if out is not None else torch.empty_like(x),
        attn_spatial=lambda qkv, n, HW, C, scale, out=None, x3h=False: out if out is not None else _e(n * HW, C),
        softmax_rows_=lambda x, rows, n, scale=1.0: x,
        vq_argmin=lambda z, Ep, esq, D, Kc: torch.zeros(z.numel() // D, dtype=torch.int64),
        vq_argmin_filtered=lambda z, blob, D, Kc, stats=None: torch.zeros(z.numel() // D, dtype=torch.int64),
        codebook_gather=lambda E, idx, D, Kc: _e(idx.numel(), D),
        halo_gn_slots=_slots,
        new_gn_part=lambda n, Hout, Wout, device: _e(n, _slots(Hout, Wout), 32, 2))
    for name, fn in stubs.items():
        monkeypatch.setattr(ops, name, rec.wrap(name, getattr(ops, name), fn))
    monkeypatch.setattr(ops, 'packed_floats', _pf)                                      # (a size, not a launch)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda device=None: None)


_WEIGHTS = {}


def _weights(cfg):
    """a state dict of the configuration's shapes; the recorder reads shapes only, so every tensor of one shape is one untouched buffer"""
    import numpy as np
    from viewformer_amd.weights import vqgan_layout
    from viewformer_amd.vqgan import VQGAN
    key = json.dumps(cfg.asdict(), sort_keys=True)
    if key not in _WEIGHTS:
        shapes = {}

        def conv(name, cin, cout, k):
            shapes[name + '.weight'], shapes[name + '.bias'] = (cout, cin, k, k), (cout,)

        def norm(name, c):
            shapes[name + '.weight'], shapes[name + '.bias'] = (c,), (c,)
        for kind, name, args in sum(vqgan_layout(cfg), []):
            if kind in ('conv3', 'down', 'up'):
                conv(name, args[0], args[1], 3)
            elif kind == 'res':
                norm(name + '.norm1', args[0]); conv(name + '.conv1', args[0], args[1], 3)
                norm(name + '.norm2', args[1]); conv(name + '.conv2', args[1], args[1], 3)
                if args[0] != args[1]:
                    conv(name + '.nin_shortcut', args[0], args[1], 1)
            elif kind == 'attn':
                norm(name + '.norm', args[0])
                for p in ('q', 'k', 'v', 'proj_out'):
                    conv(f'{name}.{p}', args[0], args[0], 1)
            elif kind == 'norm_swish':
                norm(name, args[0])
        conv('quant_conv', cfg.z_channels, cfg.embed_dim, 1)
        conv('post_quant_conv', cfg.embed_dim, cfg.z_channels, 1)
        shapes['quantize.embeddings'] = shapes['quantize.ema_dw_hidden'] = (cfg.embed_dim, cfg.n_embed)
        shapes['quantize.ema_cluster_size_hidden'] = (cfg.n_embed,)
        sd = {k: np.zeros(s, np.float32) for k, s in shapes.items()}
        sd['quantize.counter'] = np.zeros((), np.int64)
        assert sorted(sd) == sorted(VQGAN(cfg).expected_keys())
        _WEIGHTS[key] = sd
    return _WEIGHTS[key]


def _model(monkeypatch, cfg_kw, ctor, attrs):
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.vqgan import VQGAN
    cfg = VQGANConfig(**cfg_kw)
    attrs = dict(attrs)
    if 'VF_VQ_DENSE_X3H' in attrs:
        monkeypatch.setenv('VF_VQ_DENSE_X3H', attrs.pop('VF_VQ_DENSE_X3H'))
    else:
        monkeypatch.delenv('VF_VQ_DENSE_X3H', raising=False)
    m = VQGAN(cfg, data_format='NHWC', **ctor).load_state_dict(_weights(cfg))
    for k, v in attrs.items():
        assert hasattr(VQGAN, k), k
        setattr(m, k, v)
    m.device = torch.device('cpu')
    return m


def _refusals(m, rec):
    """the bf16-activation refusals, each as ['raises', text] behind the launches issued before it"""
    from viewformer_amd import ops
    from viewformer_amd._lib import VfError
    x16 = torch.zeros((16 * 16, 512), dtype=torch.bfloat16)
    x32 = torch.zeros((16 * 16, 512))
    x8 = torch.zeros((8 * 8, 512), dtype=torch.bfloat16)
    xq = torch.zeros((64, m.config.z_channels), dtype=torch.bfloat16)
    tries = (lambda: m._gn(x16, 'decoder.mid.block_1.norm1', 1, 256, 512),                       # no partial statistics for a bf16 activation
             lambda: m._conv3(x32, 'encoder.mid.block_1.conv1', 1, 16, 16, o16=True),            # an encoder layer has no bf16 packing
             lambda: m._conv3(x16, 'decoder.mid.block_1.conv1', 1, 16, 16),                      # bf16 in on the layer's own arm
             lambda: m._conv3(x8, 'decoder.mid.block_1.conv1', 1, 8, 8),                         # ... below the halo shape
             lambda: m._conv3(x16, 'decoder.up.4.upsample.conv', 1, 16, 16, mode=ops.MODE_CONV3_UP2),
             lambda: m._conv1(xq, 'quant_conv', 64),                                             # an encoder 1x1
             lambda: m._conv1(x16, 'decoder.mid.attn_1.proj_out', 256, res=x16),                 # bf16 GEMM with a residual
             lambda: m._conv1(x16, 'decoder.mid.attn_1.proj_out', 256),
             lambda: m._conv1(x16, 'decoder.mid.attn_1.proj_out', 256, pro=(x32, x32, x32)))
    for t in tries:
        try:
            t()
            rec.calls.append(['returns'])
        except VfError as e:
            rec.calls.append(['raises', str(e)])


def _convs(rec):
    """VQGANTrainer._conv_launch and LPIPS._conv on the smallest shapes on each side of their rules"""
    from viewformer_amd import ops
    from viewformer_amd.lpips import LPIPS
    from viewformer_amd.vqgan_train import VQGANTrainer
    S1, S2, UP = ops.MODE_CONV3_S1, ops.MODE_CONV3_S2PAD, ops.MODE_CONV3_UP2
    out = {}
    #       cin cout k  H   W  mode
    rows = ((32, 128, 3, 8, 16, S1), (32, 128, 3, 8, 8, S1), (32, 128, 3, 4, 16, S1), (32, 64, 3, 8, 16, S1), (16, 128, 3, 8, 16, S1),
            (32, 128, 3, 16, 32, S2), (32, 128, 3, 16, 16, S2), (32, 128, 3, 4, 8, UP), (32, 128, 3, 4, 4, UP),
            (32, 3, 3, 8, 32, S1), (32, 3, 3, 8, 16, S1), (32, 5, 3, 8, 32, S1), (704, 3, 3, 8, 32, S1),
            (64, 64, 1, 4, 4, 0), (32, 64, 1, 4, 4, 0), (64, 32, 1, 4, 4, 0))
    for cin, cout, k, H, W, mode in rows:
        Ho, Wo = (H // 2, W // 2) if mode == S2 else (H * 2, W * 2) if mode == UP else (H, W)
        w, b, x = torch.zeros(cout, cin, k, k), torch.zeros(cout), torch.zeros(2 * H * W, cin)
        for act in (False, True):
            for res in (None, torch.zeros(2 * Ho * Wo, cout)):
                rec.reset()
                y, ho, wo = VQGANTrainer._conv_launch(None, x, w, b, 2, H, W, mode, res=res, activations=act)
                assert (tuple(y.shape), ho, wo) == ((2 * Ho * Wo, cout), Ho, Wo)
                out[f'trainer/{cin}x{cout}k{k}/{H}x{W}/mode{mode}/act={act}/res={res is not None}'] = rec.calls
        if k == 3 and mode == S1:
            cache = {}
            for i, act in enumerate((False, True, True, False)):                       # the second pair finds its packing in the cache
                rec.reset()
                y = LPIPS._conv(x, w, b, cache, 2, H, W, activations=act)
                assert tuple(y.shape) == (2 * H * W, cout)
                out[f'lpips/{cin}x{cout}/{H}x{W}/{i}/act={act}'] = rec.calls
            out[f'lpips/{cin}x{cout}/{H}x{W}/cache'] = [sorted(cache)]
    return out


def record(monkeypatch):
    rec = CodecRecorder()
    _patch(monkeypatch, rec)
    out = {}

    def seq(name, fn):
        rec.reset()
        res = fn()
        out[name] = rec.calls
        return res

    for name, (cfg_kw, ctor, attrs, n, side) in CASES.items():
        m = _model(monkeypatch, cfg_kw, ctor, attrs)
        seq(name + '/upload', m._upload)
        codes = seq(name + '/encode', lambda: m.encode(torch.zeros((n, side, side, 3), dtype=torch.uint8))[-1])
        assert tuple(codes.shape) == (n, side // m.config.stride, side // m.config.stride)
        img = seq(name + '/decode_code', lambda: m.decode_code(codes))
        assert tuple(img.shape) == (n, side, side, 3) and img.dtype == torch.float32
        if name.startswith('default/') or name in ('fuse_gn_stats=False/bf16', 'VF_VQ_DENSE_X3H=0/bf16'):
            seq(name + '/refusals', lambda: _refusals(m, rec))
        del m
        rec.keep.clear()
    out.update(_convs(rec))
    return out


def test_the_codec_issues_the_recorded_launches(monkeypatch):
    got = json.loads(json.dumps(record(monkeypatch)))
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert sorted(got) == sorted(want)
    for name in want:
        if name.endswith('/cache'):
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
        one = lambda n, v: json.dumps(v if n.endswith('/cache') else [digest(c) for c in v], separators=(',', ':'))      # noqa: E731
        print('{' + ',\n'.join('"%s":%s' % (n, one(n, v)) for n, v in rec.items()) + '}')
