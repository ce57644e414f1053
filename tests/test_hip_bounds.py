"""GPU: the memory footprint of the kernels (the contract at the top of include/vf_hip.h).

Every case of the table runs the same call four ways:
  A  compact   plain contiguous tensors, as the other test files call it
  B  framed    every input and output inside a tests/framed.py Frame: padded strides (the smallest pad the entry point's alignment allows:
               4 fp32 / 8 bf16 elements), NaN sentinels in every gap and guard.  No frame may report a violation — outputs written exactly
               on their logical elements, inputs and guards untouched — and the logical outputs equal run A bit for bit.
  C  selection kernels only: B again with the input guards refilled with +3e38, then -3e38 (a comparison ignores NaN).
  D  positive control, one per family: the output frame is declared one column narrower than the kernel is told; violations() must report
     exactly that column of every row — the check sees this kernel's stores.

No entry point of this table documents a routing that depends on a stride or an alignment the frames change (pads keep every row 16-byte
aligned, interior pointers are 256-byte aligned), so A and B always take the same kernel and are compared bit for bit.

Shapes are the smallest at which each property can fail; where an entry point refuses a listed shape the nearest accepted one is used:
  * vf_igemm_f32 has no tile selector (vf_select has none for it): the 64x64-tile variant is taken for Cout % 64 == 0 on an under-filled
    grid, so (200, 64, 64) runs the 64-column kernel, (200, 64, 192) the 64x64 variant and (130, 96, 160) the 128x128 one.
  * bf16 activations (a16 / o16, hence the whole 256-tile kernel) need Cin % 128 == 0: K = 128 instead of 64 there.
  * vf_conv3_halo_bf16 refuses bf16 activations on the 8x8 pair geometry: that form runs on the 8x16 / 16x16 tiles only.
  * vf_camera_knn_workspace_bytes is 0 up to N = 1024 (one launch writes the result): N = 1500 is added for the workspace.
  * vf_igemm_f32 (the f32 halo kernel behind it) refuses gn_part: the fused GroupNorm partials are framed for the x6 / bf16 / x3h kernels.
  * the training attention's streams mask needs whole streams: (B, H, S, L) = (2, 2, 3, 64) is 3 streams of S = 3 views, T = 576.
  * kernels behind a vf_select switch run on both sides of it where the shape reaches both (x3h convolution MFMA shape, LDS-DMA attention
    32- / 64-query waves and the register-staged kernel, the 128-tile GEMM at the 256-tile shapes, LayerNorm backward one / two rows).

After a failed GPU call (a HIP error, not a refused argument) the session is ended: nothing more is started on a device that has faulted.
"""
import ctypes

import numpy as np
import pytest
import torch

from framed import Frame, ROW_GAP

pytestmark = pytest.mark.gpu

F32, BF16, U8, I32, I64, F64 = torch.float32, torch.bfloat16, torch.uint8, torch.int32, torch.int64, torch.float64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale + shift).astype(np.float32))


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib_():
    from viewformer_amd import _lib
    return _lib.load()


def _ok(status, what):
    from viewformer_amd import _lib
    _lib.check(status, what)


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------ allocation: compact or framed
class Alloc:
    """hands a case its tensors: plain contiguous ones (run A) or windows of sentinel-filled frames with padded strides (runs B, C, D)"""

    def __init__(self, dev, framed, fill=None, narrow=None):
        self.dev, self.framed, self.fill, self.narrow = dev, framed, fill, narrow
        self.frames = {}            # name -> (Frame, kind)
        self.keep = []              # compact tensors stay alive until the case has run (a case may pass only their pointers on)

    def _frame(self, name, kind, shape, dtype, pad, bpad):
        assert name not in self.frames, name
        shape = tuple(int(s) for s in shape)
        batch, rows, cols = (1, 1, shape[0]) if len(shape) == 1 else (1,) + shape if len(shape) == 2 else shape
        ld = cols + pad
        cols_decl = cols - 1 if name == self.narrow else cols
        f = Frame(rows, cols_decl, ld, dtype, self.dev, batch=batch, batch_stride=rows * ld + bpad,
                  **(dict(guard_rows=0) if len(shape) == 1 else {}))                     # (a flat buffer has no rows: 1 MiB guards)
        self.frames[name] = (f, kind)
        v = f.widened(cols) if name == self.narrow else f.view
        return f, (v[0] if len(shape) == 1 else v)

    def inp(self, name, t, pad=0, bpad=0):
        """an input: 1-D [n], 2-D [rows, cols] or 3-D [batch, rows, cols]; ``pad`` elements behind every row, ``bpad`` behind every batch entry"""
        if not self.framed:
            self.keep.append(t.to(self.dev).contiguous().clone())
            return self.keep[-1]
        f, v = self._frame(name, 'in', t.shape, t.dtype, pad, bpad)
        f.load(t.reshape(f.view.shape))
        if self.fill is not None and t.dtype.is_floating_point:
            f.refill(self.fill)
        return v

    def out(self, name, shape, dtype=F32, pad=0, bpad=0, init=None):
        """an output every logical element of which the kernel writes; ``init``: an accumulating (read-modify-write) output's start value"""
        if not self.framed:
            self.keep.append(torch.empty(shape, dtype=dtype, device=self.dev) if init is None
                             else init.to(self.dev).to(dtype).reshape(shape).contiguous().clone())
            return self.keep[-1]
        f, v = self._frame(name, 'out', shape, dtype, pad, bpad)
        if init is not None:
            f.load(init.reshape(f.view.shape), accumulate=True)
        return v

    def ws(self, name, nbytes):
        """a workspace of exactly the advertised size (None for 0 bytes): written only inside, not necessarily everywhere"""
        if nbytes == 0:
            return None
        if not self.framed:
            self.keep.append(torch.empty(nbytes, dtype=U8, device=self.dev))
            return self.keep[-1]
        f = Frame.raw(nbytes, self.dev)
        self.frames[name] = (f, 'ws')
        return f.view

    def check(self):
        torch.cuda.synchronize()
        bad = {}
        for name, (f, kind) in self.frames.items():
            v = f.violations()
            if kind == 'ws':
                v = [x for x in v if x[0] != 'unwritten']
            if name == self.narrow:
                want = torch.tensor([b * f.batch_stride + r * f.ld + f.cols for b in range(f.batch) for r in range(f.rows)])
                got = f.offsets(ROW_GAP)
                assert torch.equal(got, want), f'positive control {name}: the withheld column {f.cols} of {f.rows * f.batch} rows expected in the row ' \
                                               f'gap, got {got.numel()} elements, first {got[:8].tolist()}'
                v = [x for x in v if x[0] != ROW_GAP]
            if v:
                bad[name] = v
        assert not bad, f'footprint violations (region, first offset, count): {bad}'


class Case:
    def __init__(self, cid, family, make, selection=False, control=None, select=None):
        self.id, self.family, self.make, self.selection, self.control, self.select = cid, family, make, selection, control, select


CASES = []


def case(cid, family, make, **kw):
    assert cid not in [c.id for c in CASES], cid
    CASES.append(Case(cid, family, make, **kw))


def _run(c, dev, alloc):
    from viewformer_amd import _lib
    prev = [(w, _lib.select(w, v)) for w, v in (c.select or [])]
    try:
        outs = c.fn(alloc)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if isinstance(e, _lib.VfError) and 'HIP error' not in str(e):
            raise                                           # an argument the entry point refused before any launch
        pytest.exit(f'{c.id}: a GPU call failed, nothing more is started on this device: {e}', returncode=3)
    finally:
        for w, p in prev:
            _lib.select(w, p)
    return outs


def _same(got, ref, what):
    assert got.keys() == ref.keys()
    for k in ref:
        g, r = _bits(got[k]), _bits(ref[k])
        assert g.shape == r.shape and torch.equal(g, r), f'{what}: output {k} differs from the compact run in {(g != r).sum().item()} of {r.numel()} elements'


_prepared = {}


def _prepare(c, dev):
    if c.id not in _prepared:
        _prepared.clear()                                   # one case's operands alive at a time
        c.fn = c.make(dev)
        _prepared[c.id] = {k: v.clone() for k, v in _run(c, dev, Alloc(dev, False)).items()}        # run A, computed once per case
    return _prepared[c.id]


# ================================================================================================ dense
def _gemm(kind, M, K, N, full, a16=False, o16=False, sel=None, control=None, tag=''):
    def make(dev):
        from viewformer_amd import ops
        w = _rand((K, N), 2, 0.1).to(dev)
        wp = {'f32': ops.pack_dense_kn, 'bf16': ops.pack_dense_kn_bf16, 'x6': ops.pack_dense_kn_x6, 'x3h': ops.pack_dense_kn_x3h}[kind](w)
        x = _rand((M, K), 1).to(BF16 if a16 else F32)
        bias, res = _rand((N,), 3), _rand((M, N), 4)
        flags = dict(bf16=kind == 'bf16', x6=kind == 'x6', x3h=kind == 'x3h', a16=a16, o16=o16)

        def fn(A):
            xv = A.inp('x', x, pad=8 if a16 else 4)
            out = A.out('out', (M, N), BF16 if o16 else F32, pad=8 if o16 else 4)
            b = A.inp('bias', bias) if full else None
            r = A.inp('res', res, pad=4) if full and not o16 else None
            ops.igemm(xv, A.inp('w', wp), M, K, N, out, bias=b, res=r, epilogue=ops.EPI_GELU if full else ops.EPI_NONE,
                      lda=xv.stride(0), ldc=out.stride(0), ldr=r.stride(0) if r is not None else None, **flags)
            return {'out': out}
        return fn
    case(f'gemm_{kind}{tag}-{M}x{K}x{N}-{"gelu_bias_res" if full else "plain"}' + ('-a16' if a16 else '') + ('-o16' if o16 else ''),
         f'gemm_{kind}', make, select=sel, control=control)


for _full in (False, True):
    _gemm('f32', 1, 32, 3, _full)                                                      # one row; N below a float4
    _gemm('f32', 200, 64, 64, _full, control=None if _full else 'out')                 # ragged against the tiles; 64-column kernel
    _gemm('f32', 200, 64, 192, _full)                                                  # the 64x64-tile variant of the 128-wide packing
    _gemm('f32', 130, 96, 160, _full)                                                  # ragged M and a 32-column N tail, 128x128 tiles
    _gemm('bf16', 1, 64, 128, _full)
    _gemm('bf16', 200, 64, 160, _full, control=None if _full else 'out')
    for _kind in ('x3h', 'x6'):
        _gemm(_kind, 1, 64, 3, _full)
        _gemm(_kind, 200, 64, 160, _full, control=None if _full else 'out')
for _a16 in (False, True):
    for _o16 in (False, True):
        _gemm('bf16', 129, 128, 128, True, a16=_a16, o16=_o16)                         # paired bf16 stores on an odd last row


def _gemm_batched_qk(dev):
    """the batched q.k^T of test_gemm_strided_views_and_batch, slabs of the output 64 floats apart"""
    from viewformer_amd import ops
    n, HW, C = 3, 64, 64
    qkv = _rand((n * HW, 3 * C), 7)
    kp = ops.pack(qkv.to(dev)[:, C:2 * C], C, HW, 1, sk=1, sn=3 * C, st=0, batch=n, src_bstride=HW * 3 * C)

    def fn(A):
        x = A.inp('qkv', qkv, pad=4)
        out = A.out('S', (n, HW, HW), pad=4, bpad=64)
        ops.igemm(x[:, :C], A.inp('kp', kp), HW, C, HW, out, lda=x.stride(0), ldc=out.stride(1), batch=n, stride_x=HW * x.stride(0),
                  stride_w=ops.packed_floats(C, HW), stride_out=out.stride(0))
        return {'S': out}
    return fn


case('gemm_f32-batched_qk-batch_gap', 'gemm_f32', _gemm_batched_qk)


def _gemm_x6_splitk(dev):
    from viewformer_amd import ops
    M, K, N, S = 200, 384, 160, 3
    x = _rand((M, K), 1)
    wp = ops.pack_dense_kn_x6(_rand((K, N), 2, 0.1).to(dev))

    def fn(A):
        xv = A.inp('x', x, pad=4)
        out = A.out('slabs', (S, M, N), bpad=64)                                        # stride_out = M * Cout + 64: the slab gap
        ops.igemm(xv, A.inp('w', wp), M, K, N, out, lda=xv.stride(0), x6=True, split_k=S, stride_out=out.stride(0))
        return {'slabs': out}
    return fn


case('gemm_x6-splitk3-slab_gap', 'gemm_x6', _gemm_x6_splitk)


def _gemm_g256(M, form, sel=None, tag=''):
    K, N = 128, 256

    def make(dev):
        from viewformer_amd import ops
        assert ops.gemm_g256_shape_ok(M, K, N)
        wp = ops.pack_dense_kn_bf16(_rand((K, N), 2, 0.1).to(dev))
        x, bias, res = _rand((M, K), 1).to(BF16), _rand((N,), 3), _rand((M, N), 4)

        def fn(A):
            xv, w, b = A.inp('x', x, pad=8), A.inp('w', wp), A.inp('bias', bias)
            kw = dict(lda=xv.stride(0), bf16=True, a16=True)
            if form == 'f32_res':
                out, r = A.out('out', (M, N), pad=4), A.inp('res', res, pad=4)
                ops.igemm(xv, w, M, K, N, out, bias=b, res=r, ldc=out.stride(0), ldr=r.stride(0), **kw)
            elif form == 'o16':
                out = A.out('out', (M, N), BF16, pad=8)
                ops.igemm(xv, w, M, K, N, out, bias=b, ldc=out.stride(0), o16=True, **kw)
            elif form == 'dual':
                out, aux = A.out('out', (M, N), pad=8), A.out('aux', (M, N), BF16, pad=8)
                ops.igemm(xv, w, M, K, N, out, bias=b, ldc=out.stride(0), epilogue=ops.EPI_GELU_DUAL, out_aux=aux, **kw)
                return {'out': out, 'aux': aux}
            elif form == 'gelu_bwd_res16':
                out, r = A.out('out', (M, N), BF16, pad=8), A.inp('u16', res.to(BF16), pad=8)
                ops.igemm(xv, w, M, K, N, out, res=r, ldc=out.stride(0), ldr=r.stride(0), epilogue=ops.EPI_GELU_BWD, o16=True, res16=True, **kw)
            else:
                out, r = A.out('out', (M, N), pad=4), A.inp('res', res, pad=4)
                ops.igemm(xv, w, M, K, N, out, bias=b, res=r, ldc=out.stride(0), ldr=r.stride(0), drop=(0.1, 9, 3), **kw)
            return {'out': out}
        return fn
    case(f'gemm_g256{tag}-{M}x{K}x{N}-{form}', 'gemm_bf16' if sel else 'gemm_g256', make, select=sel, control=None if sel else 'out' if (M, form) == (257, 'o16') else ('aux' if (M, form) == (320, 'dual') else None))


for _M in (256, 257, 320):                                                             # exact; one row / 64 rows in the last 256-row tile
    for _form in ('f32_res', 'o16', 'dual', 'gelu_bwd_res16', 'drop'):
        _gemm_g256(_M, _form)
    for _form in ('f32_res', 'o16'):                                                    # VF_SEL_GEMM_G256 = 0: the 128-tile kernel on bf16 activations
        _gemm_g256(_M, _form, sel=[(1, 0)], tag='_off')


def _gemm_tn(M, splits, y16, with_bias):
    K, N = 256, 256

    def make(dev):
        x, dy = _rand((M, K), 1).to(BF16), _rand((M, N), 2, 0.1).to(BF16 if y16 else F32)
        rec = K * N + (N if with_bias else 0)

        def fn(A):
            xv, dv = A.inp('x', x, pad=8), A.inp('dy', dy, pad=8 if y16 else 4)
            ws = A.out('w_slabs', (splits * rec,))                                     # exactly splits * rec floats: weight slab | bias slab
            _ok(_lib_().vf_gemm_tn_bf16(_P(xv), xv.stride(0), _P(dv), 1 if y16 else 0, dv.stride(0), M, K, N, splits, _P(ws),
                                        ctypes.c_void_p(ws.data_ptr() + K * N * 4) if with_bias else None, rec, _strm()), 'vf_gemm_tn_bf16')
            return {'w_slabs': ws}
        return fn
    case(f'gemm_tn-{M}x{K}x{N}-splits{splits}-{"dy16" if y16 else "dy32"}-{"bias" if with_bias else "nobias"}', 'gemm_tn', make,
         control='w_slabs' if (splits, y16, with_bias) == (3, False, True) else None)


for _M, _sp in ((64, 1), (192, 3)):
    for _y16 in (False, True):
        for _wb in (False, True):
            _gemm_tn(_M, _sp, _y16, _wb)


def _sum_slabs(n, acc):
    def make(dev):
        slabs, d0 = _rand((3, 1, n), 1), _rand((n,), 2)

        def fn(A):
            s = A.inp('slabs', slabs, bpad=8)                                          # ld = n + 8 > n
            dst = A.out('dst', (n,), init=d0 if acc else None)
            _ok(_lib_().vf_sum_slabs_f32(_P(s), 3, s.stride(0), n, _P(dst), 1 if acc else 0, _strm()), 'vf_sum_slabs_f32')
            return {'dst': dst}
        return fn
    case(f'sum_slabs-n{n}-{"acc" if acc else "set"}', 'sum_slabs', make, control='dst' if (n, acc) == (1028, False) else None)


for _n in (4, 1028):
    for _acc in (False, True):
        _sum_slabs(_n, _acc)


# ================================================================================================ convolutions
def _conv(kind, mode, cin, cout, Hin, Win, n, pro=False, res=False, gn=False, a16=False, o16=False, sel=None, control=None, tag=''):
    def make(dev):
        from viewformer_amd import ops
        m = {'s1': ops.MODE_CONV3_S1, 's2': ops.MODE_CONV3_S2PAD, 'up': ops.MODE_CONV3_UP2}[mode]
        Ho, Wo = {'s1': (Hin, Win), 's2': (Hin // 2, Win // 2), 'up': (Hin * 2, Win * 2)}[mode]
        M = n * Ho * Wo
        w = _rand((cout, cin, 3, 3), 12, 0.05).to(dev)
        wp = {'f32': ops.pack_conv_oihw, 'bf16': ops.pack_conv3_bf16, 'x6': ops.pack_conv3_x6, 'x3h': ops.pack_conv3_x3h}[kind](w)
        x32 = _rand((n * Hin * Win, cin), 11, 1.4, 0.2)
        x = x32.to(BF16) if a16 else x32
        bias, gamma, beta = _rand((cout,), 13), _rand((cin,), 14, 0.3, 1.0), _rand((cin,), 15, 0.2)
        r0 = _rand((M, cout), 16).to(BF16 if o16 else F32)
        stats = ops.groupnorm_stats(x.float().to(dev), gamma.to(dev), n, Hin * Win, cin) if pro else None
        flags = dict(bf16=kind == 'bf16', x6=kind == 'x6', x3h=kind == 'x3h', a16=a16, o16=o16)
        slots = ops.halo_gn_slots(Ho, Wo) if gn else 0

        def fn(A):
            xv = A.inp('x', x)                                                         # NHWC: the convolutions take no input stride
            out = A.out('out', (M, cout), BF16 if o16 else F32, pad=8 if o16 else 4)
            r = A.inp('res', r0, pad=8 if o16 else 4) if res else None
            p = (A.inp('pro_mean', stats[0]), A.inp('pro_scale', stats[1]), A.inp('pro_beta', beta)) if pro else None
            part = A.out('gn_part', (n * slots * 64,)) if gn else None                 # exactly [n][slots][32][2]
            ops.igemm(xv, A.inp('w', wp), M, cin, cout, out, bias=A.inp('bias', bias), res=r, mode=m, pro=p, pro_swish=True, Hin=Hin, Win=Win, Hout=Ho,
                      Wout=Wo, ldc=out.stride(0), ldr=r.stride(0) if res else None, gn_part=part.view(n, slots, 32, 2) if gn else None, **flags)
            return {'out': out, 'gn_part': part} if gn else {'out': out}
        return fn
    case(f'conv_{kind}{tag}-{mode}-{cin}to{cout}-{Hin}x{Win}-n{n}' + ('-pro' if pro else '') + ('-res' if res else '') + ('-gn' if gn else '')
         + ('-a16' if a16 else '') + ('-o16' if o16 else ''), f'conv_{kind}', make, select=sel, control=control)


# the per-tap f32 kernel, 3 images
_conv('f32', 's1', 64, 3, 16, 16, 3, tag='_pertap', control='out')
_conv('f32', 's2', 64, 64, 16, 16, 3, res=True, tag='_pertap')
_conv('f32', 'up', 64, 32, 8, 8, 3, tag='_pertap')
# the halo kernels, Cin 32 -> Cout 128, GroupNorm + swish prologue on: one 8x16 tile, 16x16 with two images, upsample from 4x8, and the
# pair geometry with THREE 8x8 images (the duplicate half-tile must neither store an image 3 nor let image-3 bytes reach images 0-2)
_HALO = [('s1', 8, 16, 1), ('s1', 16, 16, 2), ('up', 4, 8, 1), ('up', 4, 8, 2), ('s1', 8, 8, 3)]
for _mode, _H, _W, _n in _HALO:
    _pair = (_H, _W) == (8, 8)
    _conv('f32', _mode, 32, 128, _H, _W, _n, pro=True, res=True, tag='_halo', control='out' if _pair else None)
    _conv('x6', _mode, 32, 128, _H, _W, _n, pro=True, res=True, gn=True, control='out' if _pair else None)
    _conv('bf16', _mode, 32, 128, _H, _W, _n, pro=True, res=True, gn=True, control='gn_part' if _pair else None)
    if not _pair:
        _conv('bf16', _mode, 32, 128, _H, _W, _n, pro=True, res=True, gn=True, a16=True, o16=True, control='out' if _n == 2 and _mode == 's1' else None)
    for _k32 in (1, 0):                                                                # both MFMA shapes of the x3h convolution
        _conv('x3h', _mode, 32, 128, _H, _W, _n, pro=True, res=True, gn=True, sel=[(4, _k32)], tag=f'_k32is{_k32}',
              control='out' if _pair and _k32 else None)
_conv('x3h', 's2', 32, 128, 16, 16, 3, res=True, gn=True, tag='_pair_s2')                # 16x16 -> 8x8 stride 2: two images per tile, odd count
_conv('x6', 's2', 32, 128, 16, 32, 1, res=True, gn=True)


def _small_cout(cout, n, x16):
    cin, H, W = 32, 8, 32

    def make(dev):
        from viewformer_amd import ops
        x32 = _rand((n * H * W, cin), 51, 1.4, 0.2)
        w, b, gamma, beta = _rand((cout, cin, 3, 3), 52, 0.05), _rand((cout,), 53), _rand((cin,), 54, 0.3, 1.0), _rand((cin,), 55, 0.2)
        x = x32.to(BF16) if x16 else x32
        stats = ops.groupnorm_stats(x.float().to(dev), gamma.to(dev), n, H * W, cin)

        def fn(A):
            out = A.out('out', (n * H * W, cout))                                      # 4 * Cout bytes per pixel next to 16-byte stores
            ops.conv3_small_cout(A.inp('x', x), A.inp('w', w.reshape(-1)), A.inp('bias', b), n, H, W, cin, cout,
                                 pro=(A.inp('pro_mean', stats[0]), A.inp('pro_scale', stats[1]), A.inp('pro_beta', beta)), out=out)
            return {'out': out}
        return fn
    case(f'conv_small_cout-{cout}-n{n}-{"x16" if x16 else "x32"}', 'conv_small_cout', make, control='out' if (cout, n, x16) == (3, 2, False) else None)


for _co in (1, 3, 4):
    for _n in (1, 2):
        for _x16 in (False, True):
            _small_cout(_co, _n, _x16)


def _conv_in(u8, cout, x3h=False):
    n, H, W = 2, 8, 16 if x3h else 8

    def make(dev):
        from viewformer_amd import ops
        g = np.random.Generator(np.random.PCG64(41))
        img = torch.from_numpy(g.integers(0, 256, (n * H * W, 3), dtype=np.uint8))
        img = img if u8 else img.float() / 127.5 - 1
        w, b = _rand((cout, 3, 3, 3), 42, 0.2), _rand((cout,), 43)
        wp = ops.pack_conv_in_x3h(w.to(dev)) if x3h else None
        slots = ops.halo_gn_slots(H, W) if x3h else 0

        def fn(A):
            out = A.out('out', (n * H * W, cout))
            part = A.out('gn_part', (n * slots * 64,)) if x3h else None
            ops.conv_in(A.inp('img', img), A.inp('w', w.reshape(-1)), A.inp('bias', b), n, H, W, cout, out=out, wp3h=A.inp('wp', wp) if x3h else None,
                        gn_part=part.view(n, slots, 32, 2) if x3h else None)
            return {'out': out, 'gn_part': part} if x3h else {'out': out}
        return fn
    case(f'conv_in{"_x3h" if x3h else ""}-{"u8" if u8 else "f32"}-{cout}', 'conv_in', make, control='out' if (u8, cout) == (True, 4) else None)


for _u8 in (True, False):
    _conv_in(_u8, 4)
    _conv_in(_u8, 32)
    _conv_in(_u8, 128, x3h=True)


def _wgrad(splits):
    mode, cin, cout, n, h, w = 1, 128, 132, 4, 8, 8                                     # the last case of test_conv3_wgrad_kernel_matches_autograd

    def make(dev):
        from viewformer_amd import ops
        x, dy = _rand((n * h * w, cin), 1), _rand((n * h * w, cout), 2)
        dyp = ops.pack_dense_kn_x6(dy.to(dev))
        rows = int(_lib_().vf_conv3_wgrad_x6_rows(cin))

        def fn(A):
            slabs = A.out('slabs', (splits * rows * cout,))                            # exactly splits x rows x Cout
            _ok(_lib_().vf_conv3_wgrad_x6(_P(A.inp('x', x)), _P(A.inp('dyp', dyp)), _P(slabs), n, h, w, cin, h, w, cout, mode, splits, _strm()),
                'vf_conv3_wgrad_x6')
            return {'slabs': slabs}
        return fn
    case(f'conv_wgrad-splits{splits}', 'conv_wgrad', make, control='slabs' if splits == 2 else None)


_wgrad(1)
_wgrad(2)


# ================================================================================================ attention
def _attn_fwd(kind, L, S, twin, in16=False, o16=False, control=None, sel=None, tag=''):
    B, H = 2, 2
    d, T = H * 64, S * L

    def make(dev):
        from viewformer_amd import ops
        qkv = _rand((B * T, 3 * d), 71, 0.35).to(BF16 if in16 else F32)
        kw = dict(bf16=kind == 'bf16', x6=kind == 'x6', fp8=kind == 'fp8')

        def fn(A):
            g = A.inp('qkv', qkv, pad=8)                                               # q, k, v = thirds of ONE buffer [B*T][3d + 8]
            out = A.out('out', (B * T, d), BF16 if o16 else F32, pad=8)
            ld = g.stride(0)
            ops.attn_blockcausal(g[:, d:2 * d], g[:, 2 * d:], g[:, :d], out, B, H, T, L, ld, ld, ld, out.stride(0), 1.0, True, S - 2 if twin else -1, **kw)
            return {'out': out}
        return fn
    case(f'attn_{kind}{tag}-L{L}-S{S}-{"twin" if twin else "causal"}' + ('-in16' if in16 else '') + ('-o16' if o16 else ''), f'attn_{kind}', make,
         control=control, select=sel)


for _kind in ('f32', 'x6', 'bf16', 'fp8'):
    for _L, _S in ((16, 3), (48, 3), (64, 5)):                                         # T = 48 < one query tile; 144 ragged vs 128 / 64; 320 vs 256
        for _twin in (False, True):
            _attn_fwd(_kind, _L, _S, _twin, control='out' if (_L, _twin) == (48, False) else None)
for _twin in (False, True):                                                            # bf16 tensors, 64-token views: the LDS-DMA kernel
    _attn_fwd('bf16', 64, 5, _twin, in16=True, o16=True, control=None if _twin else 'out')
    _attn_fwd('bf16', 64, 5, _twin, in16=True, o16=False)
    _attn_fwd('bf16', 64, 5, _twin, in16=True, o16=True, sel=[(3, 0)], tag='_dma_q64')      # VF_SEL_ATTN_Q32 = 0: 4 waves x 64 queries
    _attn_fwd('bf16', 64, 5, _twin, in16=True, o16=True, sel=[(0, 0)], tag='_staged')       # VF_SEL_ATTN_DMA = 0: the register-staged kernel on bf16 tensors


def _attn_train(form):
    """forward with log-sum-exp, row sums D, backward: (B, H, S, L) = (2, 2, 3, 64), streams mask (3 streams), attention dropout"""
    B, H, S, L, NS = 2, 2, 3, 64, 3
    d, T = H * 64, NS * S * L
    lo = form != 'f32'
    g16 = form == 'bf16_g16'
    dt, gdt = (BF16 if lo else F32), (BF16 if g16 else F32)
    drop = (0.1, 9, 3, 0)

    def make(dev):
        qkv, dout = _rand((B * T, 3 * d), 71, 0.35).to(dt), _rand((B * T, d), 72).to(dt)

        def fn(A):
            lib = _lib_()
            g = A.inp('qkv', qkv, pad=8)
            q, k, v, ld = g[:, d:2 * d], g[:, 2 * d:], g[:, :d], g.stride(0)
            out, lse, D = A.out('out', (B * T, d), dt, pad=8), A.out('lse', (B * H, T)), A.out('D', (B * H, T))
            do = A.inp('dout', dout, pad=8)
            gp = 8 if g16 else 4
            dq, dk, dv = (A.out(nm, (B * T, d), gdt, pad=p) for nm, p in (('dq', gp), ('dk', 2 * gp), ('dv', 3 * gp)))      # their own strides
            if lo:
                _ok(lib.vf_attn_blockcausal_bf16_lse(_P(q), _P(k), _P(v), _P(out), _P(lse), B, H, T, L, ld, ld, ld, out.stride(0), 1.0, -S, *drop, _strm()),
                    'vf_attn_blockcausal_bf16_lse')
                _ok(lib.vf_attn_bwd_prep_bf16(_P(do), _P(out), _P(D), B, H, T, do.stride(0), out.stride(0), _strm()), 'vf_attn_bwd_prep_bf16')
                _ok(lib.vf_attn_bwd_bf16(_P(q), _P(k), _P(v), _P(do), _P(lse), _P(D), _P(dq), _P(dk), _P(dv), 1 if g16 else 0, B, H, T, L, ld, ld, ld,
                                         do.stride(0), dq.stride(0), dk.stride(0), dv.stride(0), 1.0, -S, *drop, _strm()), 'vf_attn_bwd_bf16')
            else:
                _ok(lib.vf_attn_blockcausal_lse_f32(_P(q), _P(k), _P(v), _P(out), _P(lse), B, H, T, L, ld, ld, ld, out.stride(0), 1.0, 1, -S, *drop, _strm()),
                    'vf_attn_blockcausal_lse_f32')
                _ok(lib.vf_attn_bwd_prep_f32(_P(do), _P(out), _P(D), B, H, T, do.stride(0), out.stride(0), _strm()), 'vf_attn_bwd_prep_f32')
                _ok(lib.vf_attn_bwd_f32(_P(q), _P(k), _P(v), _P(do), _P(lse), _P(D), _P(dq), _P(dk), _P(dv), B, H, T, L, ld, ld, ld, do.stride(0),
                                        dq.stride(0), dk.stride(0), dv.stride(0), 1.0, -S, *drop, _strm()), 'vf_attn_bwd_f32')
            return {'out': out, 'lse': lse, 'D': D, 'dq': dq, 'dk': dk, 'dv': dv}
        return fn
    case(f'attn_train-{form}', 'attn_train', make, control={'f32': 'dk', 'bf16': 'dq', 'bf16_g16': 'dv'}[form])


for _form in ('f32', 'bf16', 'bf16_g16'):
    _attn_train(_form)


def _attn_prefix(arm, C, N):
    B, H, L = 2, 2, 64
    d = H * 64
    io16 = arm == 'bf16'
    dt = BF16 if io16 else F32

    def make(dev):
        from viewformer_amd import ops
        ctx, qq = _rand((B, C * L, 3 * d), 100 + C, 0.35).to(dt), _rand((B * N * L, 3 * d), 200 + N, 0.35).to(dt)

        def fn(A):
            g = A.inp('qkv', qq, pad=8)
            c = A.inp('cache', ctx, pad=16, bpad=64)                                   # ldkp != ldk; scenes C * L * ldkp + 64 apart: the scene gap
            out = A.out('out', (B * N * L, d), dt, pad=8)
            ld, ldp = g.stride(0), c.stride(1)
            ops.attn_prefix(g[:, d:2 * d], g[:, 2 * d:], g[:, :d], c[0][:, 2 * d:], c[0][:, :d], out, B, H, C, N, L, ld, ld, ld, ldp, ldp, c.stride(0),
                            out.stride(0), bf16=arm != 'f32eq')
            return {'out': out}
        return fn
    case(f'attn_prefix-{arm}-C{C}-N{N}', 'attn_prefix', make, control='out' if (C, N) == (2, 3) else None)


for _arm in ('bf16', 'bf16_f32io', 'f32eq'):
    for _C in (1, 2):
        for _N in (1, 3, 5):                                                           # not a multiple of the 4 (bf16) / 2 (f32eq) views per workgroup
            _attn_prefix(_arm, _C, _N)


def _attn_spatial(x3h, n):
    HW, C = 64, 256

    def make(dev):
        from viewformer_amd import ops
        qkv = _rand((n * HW, 3 * C), HW + C, 0.7)

        def fn(A):
            out = A.out('out', (n * HW, C), pad=4)
            ops.attn_spatial(A.inp('qkv', qkv, pad=4), n, HW, C, float(C ** -0.5), out=out, x3h=x3h)
            return {'out': out}
        return fn
    case(f'attn_spatial-{"x3h" if x3h else "f32"}-n{n}', 'attn_spatial', make, control='out' if (x3h, n) == (False, 3) else None)


for _x3h in (False, True):
    for _n in (1, 3):
        _attn_spatial(_x3h, _n)


# ================================================================================================ selection kernels (run C applies)
def _lmhead(M, N, h16):
    K = 128

    def make(dev):
        from viewformer_amd import ops
        wp = ops.pack_dense_nk_bf16(_rand((N, K), 91).to(dev), n_rows=N)
        h = _rand((M, K), 92).to(BF16 if h16 else F32)

        def fn(A):
            hv = A.inp('h', h, pad=8 if h16 else 4)
            idx, mx = A.out('idx', (M,), I64), A.out('max', (M,))
            _ok(_lib_().vf_lmhead_argmax_bf16(_P(hv), 1 if h16 else 0, hv.stride(0), _P(A.inp('w', wp)), M, K, N, _P(idx), _P(mx), _strm()),
                'vf_lmhead_argmax_bf16')
            return {'idx': idx, 'max': mx}
        return fn
    case(f'lmhead_argmax-M{M}-N{N}-{"h16" if h16 else "h32"}', 'lmhead_argmax', make, selection=True, control='idx' if (M, N, h16) == (65, 128, False) else None)


for _M in (1, 65, 130):
    for _N in (128, 256):
        for _h16 in (False, True):
            _lmhead(_M, _N, _h16)


def _vq_argmin(M, D, Kc):
    def make(dev):
        from viewformer_amd import ops
        z, E = _rand((M, D), 51, 0.3), _rand((D, Kc), 52, 0.3)
        Ep, esq = ops.vq_pack_codebook(E.to(dev))

        def fn(A):
            idx = A.out('idx', (M,), I64)
            _ok(_lib_().vf_vq_argmin_f32(_P(A.inp('z', z)), _P(A.inp('E_packed', Ep)), _P(A.inp('e_sq', esq)), M, D, Kc, _P(idx), _strm()), 'vf_vq_argmin_f32')
            return {'idx': idx}
        return fn
    case(f'vq_argmin-{M}x{D}x{Kc}', 'vq_argmin', make, selection=True, control='idx' if M == 130 else None)


_vq_argmin(1, 32, 64)
_vq_argmin(130, 32, 200)


def _vq_filtered(M):
    def make(dev):
        from viewformer_amd import ops
        D = 256
        Kc = next(k for k in range(32, 1025, 32) if ops.vq_filter_supported(D, k))      # the smallest codebook the filter takes
        z, E = _rand((M, D), 51, 0.3), _rand((D, Kc), 52, 0.3)
        blob = ops.vq_filter_pack(E.to(dev))

        def fn(A):
            idx = A.out('idx', (M,), I64)
            stats = A.out('stats', (4,), I32, init=torch.zeros(4, dtype=I32))             # counters: added to
            status = _lib_().vf_vq_argmin_filtered_f32(_P(A.inp('z', z)), _P(A.inp('blob', blob)), M, D, Kc, _P(idx), _P(stats), _strm())
            _ok(status, 'vf_vq_argmin_filtered_f32')
            return {'idx': idx, 'stats': stats}
        return fn
    case(f'vq_argmin_filtered-M{M}', 'vq_argmin_filtered', make, selection=True, control='idx' if M == 130 else None)


_vq_filtered(1)
_vq_filtered(130)


def _argmax_rows(dev):
    x = _rand((5, 70), 98)
    x[3, 10] = x[3, 60] = 50.0

    def fn(A):
        xv, idx = A.inp('x', x, pad=7), A.out('idx', (5,), I64)                         # ld = 77
        _ok(_lib_().vf_argmax_rows_f32(_P(xv), 5, 70, xv.stride(0), _P(idx), _strm()), 'vf_argmax_rows_f32')
        return {'idx': idx}
    return fn


case('argmax_rows-5x70-ld77', 'argmax_rows', _argmax_rows, selection=True, control='idx')


def _camera_knn(N, k):
    Q = 3

    def make(dev):
        db, qs = _rand((N, 7), 1), _rand((Q, 7), 2)
        nws = int(_lib_().vf_camera_knn_workspace_bytes(N, Q, k))
        assert (nws > 0) == (N > 1024)

        def fn(A):
            idx, dist = A.out('idx', (Q, k), I32), A.out('dist', (Q, k))
            _ok(_lib_().vf_camera_knn_f32(_P(A.inp('db', db)), N, _P(A.inp('queries', qs)), Q, k, 0.3, _P(idx), _P(dist), _P(A.ws('ws', nws)), _strm()),
                'vf_camera_knn_f32')
            return {'idx': idx, 'dist': dist}
        return fn
    case(f'camera_knn-N{N}-k{k}', 'camera_knn', make, selection=True, control='idx' if N == 130 else None)


_camera_knn(5, 5)                                                                      # N = k
_camera_knn(130, 5)
_camera_knn(1500, 5)                                                                   # two launches: candidates through the workspace


# ================================================================================================ workspace and row kernels
def _gn_stats(dev):
    n, HW, C = 3, 64, 64
    x, gamma = _rand((n * HW, C), 31, 3.0, 1.5), _rand((C,), 32, 1.0, 1.0)
    nws = int(_lib_().vf_groupnorm_workspace_bytes(n, HW, C))

    def fn(A):
        mean, scale = A.out('mean_c', (n, C)), A.out('scale_c', (n, C))
        _ok(_lib_().vf_groupnorm_stats_f32(_P(A.inp('x', x)), _P(A.inp('gamma', gamma)), n, HW, C, 32, 1e-6, _P(mean), _P(scale), _P(A.ws('ws', nws)), _strm()),
            'vf_groupnorm_stats_f32')
        return {'mean_c': mean, 'scale_c': scale}
    return fn


def _gn_finalize(dev):
    n, HW, C, slots = 3, 64, 64, 2
    g = torch.Generator().manual_seed(5)
    cnt = HW * (C // 32) / slots
    s1 = torch.randn(n, slots, 32, generator=g) * cnt ** 0.5 + 0.3 * cnt
    part = torch.stack([s1, (torch.rand(n, slots, 32, generator=g) + 0.5) * cnt + s1 * s1 / cnt], -1).reshape(-1)
    gamma = _rand((C,), 32, 1.0, 1.0)

    def fn(A):
        mean, scale = A.out('mean_c', (n, C)), A.out('scale_c', (n, C))
        _ok(_lib_().vf_groupnorm_finalize_f32(_P(A.inp('part', part)), _P(A.inp('gamma', gamma)), n, HW, C, 32, slots, 1e-6, _P(mean), _P(scale), _strm()),
            'vf_groupnorm_finalize_f32')
        return {'mean_c': mean, 'scale_c': scale}
    return fn


case('groupnorm_stats-n3-HW64-C64', 'groupnorm', _gn_stats, control='scale_c')
case('groupnorm_finalize-n3-HW64-C64', 'groupnorm', _gn_finalize)


def _gn_bwd(HW):
    n, C = 2, 64

    def make(dev):
        from viewformer_amd import ops
        x, da, gamma, beta = _rand((n * HW, C), 1, 2.0, 0.5), _rand((n * HW, C), 2), _rand((C,), 3, 0.3, 1.0), _rand((C,), 4, 0.2)
        mean, scale = ops.groupnorm_stats(x.to(dev), gamma.to(dev), n, HW, C)
        nws = int(_lib_().vf_groupnorm_bwd_workspace_bytes(n, HW, C, 32))

        def fn(A):
            dx, chan = A.out('dx', (n * HW, C)), A.out('chan_sums', (n, 2 * C))
            _ok(_lib_().vf_groupnorm_bwd_f32(_P(A.inp('x', x)), _P(A.inp('da', da)), _P(A.inp('mean_c', mean)), _P(A.inp('scale_c', scale)),
                                             _P(A.inp('gamma', gamma)), _P(A.inp('beta', beta)), _P(dx), _P(chan), n, HW, C, 32, 1e-6, 1, 0, _P(A.ws('ws', nws)),
                                             _strm()), 'vf_groupnorm_bwd_f32')
            return {'dx': dx, 'chan_sums': chan}
        return fn
    case(f'groupnorm_bwd-HW{HW}', 'groupnorm_bwd', make, control='dx' if HW == 130 else None)


_gn_bwd(48)
_gn_bwd(130)


def _colsum(acc):
    M, N = 70, 130

    def make(dev):
        x, o0 = _rand((M, N), 1), _rand((N,), 2)
        nws = int(_lib_().vf_colsum_workspace_bytes(N))

        def fn(A):
            xv, out = A.inp('x', x, pad=4), A.out('out', (N,), init=o0 if acc else None)
            _ok(_lib_().vf_colsum_f32(_P(xv), _P(out), M, N, xv.stride(0), 1 if acc else 0, _P(A.ws('ws', nws)), _strm()), 'vf_colsum_f32')
            return {'out': out}
        return fn
    case(f'colsum-70x130-ld134-{"acc" if acc else "set"}', 'colsum', make, control=None if acc else 'out')


_colsum(False)
_colsum(True)


def _ln_bwd(dev):
    rows, d = 77, 128                                                                  # (an odd row count: the two-rows-in-flight form ends on a single row)
    dy, x, gamma, g0, b0 = _rand((rows, d), 1), _rand((rows, d), 2, 2.0, 0.3), _rand((d,), 3, 1.0, 1.0), _rand((d,), 4), _rand((d,), 5)
    nws = int(_lib_().vf_layernorm_bwd_workspace_bytes(rows, d))

    def fn(A):
        dx, dg, db = A.out('dx', (rows, d)), A.out('dgamma', (d,), init=g0), A.out('dbeta', (d,), init=b0)
        _ok(_lib_().vf_layernorm_bwd_f32(_P(A.inp('dy', dy)), _P(A.inp('x', x)), _P(A.inp('gamma', gamma)), _P(dx), _P(dg), _P(db), rows, d, 1e-5, 1, None,
                                         None, 0.0, 0, 0, 0, _P(A.ws('ws', nws)), _strm()), 'vf_layernorm_bwd_f32')
        return {'dx': dx, 'dgamma': dg, 'dbeta': db}
    return fn


case('layernorm_bwd-77x128', 'layernorm_bwd', _ln_bwd, control='dx')
case('layernorm_bwd_one_row-77x128', 'layernorm_bwd', _ln_bwd, select=[(2, 0)])          # VF_SEL_LN_BWD_TWO_ROWS = 0


def _embed_bwd(dev):
    BS, L, d, vocab = 7, 16, 128, 66
    g = np.random.Generator(np.random.PCG64(91))
    ids = torch.from_numpy(g.integers(0, vocab, (BS * L,)).astype(np.int32))
    dh, wte0, wpe0 = _rand((BS * L, d), 1), _rand((vocab, d), 2), _rand((L, d), 3)
    nws = int(_lib_().vf_embed_bwd_workspace_bytes(d, vocab))

    def fn(A):
        dwte, dwpe, dadd = A.out('dwte', (vocab, d), init=wte0), A.out('dwpe', (L, d), init=wpe0), A.out('dadd', (BS, d))
        _ok(_lib_().vf_embed_bwd_f32(_P(A.inp('dh', dh)), _P(A.inp('ids', ids)), _P(dwte), _P(dwpe), _P(dadd), BS, L, d, vocab, _P(A.ws('ws', nws)), _strm()),
            'vf_embed_bwd_f32')
        return {'dwte': dwte, 'dwpe': dwpe, 'dadd': dadd}
    return fn


case('embed_bwd-BS7-L16-d128-V66', 'embed_bwd', _embed_bwd, control='dadd')


def _small_n_wgrad(acc):
    rows, K, N = 130, 256, 7

    def make(dev):
        x, dy, w0 = _rand((rows, K), 1), _rand((rows, N), 2), _rand((K, N), 3)
        slabs = int(_lib_().vf_dense_small_n_wgrad_slabs(rows))

        def fn(A):
            xv, dW = A.inp('x', x, pad=4), A.out('dW', (K, N), init=w0 if acc else None)
            _ok(_lib_().vf_dense_small_n_wgrad_f32(_P(xv), _P(A.inp('dy', dy)), _P(dW), _P(A.ws('ws', slabs * K * N * 4)), rows, K, N, xv.stride(0),
                                                   1 if acc else 0, _strm()), 'vf_dense_small_n_wgrad_f32')
            return {'dW': dW}
        return fn
    case(f'dense_small_n_wgrad-{"acc" if acc else "set"}', 'dense_small_n_wgrad', make, control=None if acc else 'dW')


_small_n_wgrad(False)
_small_n_wgrad(True)


def _image_metrics(dev):
    n, H, W, C = 2, 8, 8, 3
    g = np.random.Generator(np.random.PCG64(7))
    a, b = (torch.from_numpy(g.integers(0, 256, (n * H * W * C,), dtype=np.uint8)) for _ in range(2))
    nws = int(_lib_().vf_image_metrics_workspace_bytes(n, H, W, C))

    def fn(A):
        sums, ssim = A.out('sums', (n, 2), I64), A.out('ssim', (n,), F64)
        _ok(_lib_().vf_image_metrics_u8(_P(A.inp('a', a)), _P(A.inp('b', b)), n, H, W, C, _P(sums), _P(ssim), _P(A.ws('ws', nws)), _strm()), 'vf_image_metrics_u8')
        return {'sums': sums, 'ssim': ssim}
    return fn


case('image_metrics-2x8x8x3', 'image_metrics', _image_metrics, control='ssim')


def _l1_loss(dev):
    n = 2049
    x, y = _rand((n,), 1), _rand((n,), 2)
    np_ = int(_lib_().vf_l1_loss_partials(n))

    def fn(A):
        dy, part = A.out('dy', (n,)), A.out('part', (np_,))                             # exactly vf_l1_loss_partials(n) partial sums
        _ok(_lib_().vf_l1_loss_f32(_P(A.inp('x', x)), _P(A.inp('y', y)), _P(dy), _P(part), n, 0.5, _strm()), 'vf_l1_loss_f32')
        return {'dy': dy, 'part': part}
    return fn


case('l1_loss-n2049', 'l1_loss', _l1_loss, control='dy')


def _lpips_head(dev):
    n, HW, C = 2, 65, 64
    f0, f1, w = _rand((n * HW, C), 1), _rand((n * HW, C), 2), _rand((C,), 3).abs()
    nb = int(_lib_().vf_lpips_head_blocks(HW))

    def fn(A):
        part = A.out('part', (nb * n,))                                                # exactly vf_lpips_head_blocks(HW) x n_img
        _ok(_lib_().vf_lpips_head_f32(_P(A.inp('f0', f0)), _P(A.inp('f1', f1)), _P(A.inp('w', w)), _P(part), n, HW, C, _strm()), 'vf_lpips_head_f32')
        return {'part': part}
    return fn


case('lpips_head-HW65-C64', 'lpips_head', _lpips_head, control='part')


def _transpose(dev):
    rows, cols, batch = 70, 45, 3
    src = _rand((batch, rows, cols), 1)

    def fn(A):
        s = A.inp('src', src, pad=4, bpad=16)
        dst = A.out('dst', (batch, cols, rows), pad=4, bpad=32)                        # padded ld_dst: the tail of every output row stays untouched
        _ok(_lib_().vf_transpose_f32(_P(s), _P(dst), rows, cols, s.stride(1), dst.stride(1), batch, s.stride(0), dst.stride(0), _strm()), 'vf_transpose_f32')
        return {'dst': dst}
    return fn


case('transpose-70x45-batch3', 'transpose', _transpose, control='dst')


# ================================================================================================ the tests (after the table)
@pytest.mark.parametrize('c', CASES, ids=lambda c: c.id)
def test_kernel_footprint(dev, c):
    ref = _prepare(c, dev)
    b = Alloc(dev, True)
    got = _run(c, dev, b)
    b.check()
    _same(got, ref, 'framed (NaN guards)')
    if c.selection:
        for fill in (3e38, -3e38):
            a = Alloc(dev, True, fill=fill)
            got = _run(c, dev, a)
            a.check()
            _same(got, ref, f'guards = {fill}')


@pytest.mark.parametrize('c', [c for c in CASES if c.control], ids=lambda c: f'{c.family}:{c.id}')
def test_positive_control_sees_the_withheld_column(dev, c):
    _prepare(c, dev)
    d = Alloc(dev, True, narrow=c.control)
    _run(c, dev, d)
    assert c.control in d.frames
    d.check()


def test_every_family_has_a_positive_control():
    fam = {c.family for c in CASES}
    assert fam == {c.family for c in CASES if c.control}, fam - {c.family for c in CASES if c.control}
