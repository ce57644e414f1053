"""GPU: the inference attention kernels one by one against the float64 references of tests/infer_attention_ref.py (pinned on the CPU by
tests/test_infer_attention_ref_host.py): vf_attn_blockcausal_x6, the register-staged kernel behind vf_attn_blockcausal_bf16_v2 ("lp"),
vf_attn_blockcausal_fp8, vf_attn_prefix_bf16 / _f32eq and vf_attn_prefix_var_bf16 / _f32eq, called through the C ABI.

Rounded class.  Every output element: |got - want| <= c x unit x magnitude, unit = 2^-24 (x6, f32eq), 2^-9 (lp, prefix bf16), 2^-4 (fp8),
the magnitude as infer_attention_ref.py states it.  ``TABLE`` holds one (basis, c) per kernel: the basis is the worst error of the CPU
restatement against float64 over these very cases as the host file prints it, c = 4 x basis rounded up to a power of two — never a figure
taken from a kernel.  The bf16 kernels run every case with bf16-exact operands in two to four in / out dtype forms and once more with fp32
operands that are not bf16 numbers (the rounding of q, k, v, which the magnitude's score term is there for).

Exact class (bits): skip_masked = 1 against the dense form; twin with Vc >= the number of views against plain causal; bf16 out against the
fp32 out of the same form rounded once; bf16 in against fp32 in of the same values; vf_attn_prefix_bf16 against the register-staged
twin-mask pass over the concatenated sequence in every dtype form; vf_attn_prefix_f32eq against vf_attn_blockcausal_x6 in twin mode; VAR
with all lengths C against the fixed entry; a VAR view of length c >= 1 against the fixed entry with C = c; a VAR view against the same
launch with every cache row at or beyond its length turned to NaN; a view alone (N = 1) against the view in its batch.

Outputs are pre-filled with NaN, operands are thirds of one [rows][3d + pad] buffer (one case: separate buffers with different leading
dimensions; the prefix cache also K/V-only with ldkp != ldvp != ldq and with a prefix_stride beyond a scene's extent), and the padding
columns must still be NaN afterwards.  Refusals go through the C ABI with arguments each entry refuses before it launches anything."""
import contextlib
import ctypes
import functools
import time

import pytest
import torch

import attention_kernels_ref as A
import infer_attention_ref as I
from conftest import parity_report

pytestmark = pytest.mark.gpu

# kernel: (basis, c).  basis = worst error of the CPU restatement against float64 over the cases, in units of unit x magnitude, as
# test_infer_attention_ref_host.py measures and prints it; c = 4 x basis, rounded up to a power of two.
TABLE = {
    'x6': (1.92, 8.0),
    'lp': (0.583, 4.0),
    'fp8': (0.27, 2.0),
    'prefix bf16': (0.215, 1.0),
    'prefix f32eq': (1.69, 8.0),
}
BASIS = {k: b for k, (b, c) in TABLE.items()}
C = {k: c for k, (b, c) in TABLE.items()}
UNIT_NAME = {I.U32: '2^-24 x magnitude', I.U16: '2^-9 x magnitude', I.U8: '2^-4 x magnitude'}

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
NAN = float('nan')
BF, F32 = torch.bfloat16, torch.float32
D = I.PREFIX_H * I.DH
_worst = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    t0 = time.time()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        if k in C:
            parity_report(test='infer_attention', kernel=k, worst_ratio=_worst[k], c=C[k], basis=BASIS[k], unit=UNIT_NAME[I.UNIT[k]])
        else:
            parity_report(test='infer_attention', kernel=k, worst_ratio=_worst[k], c=0, basis=0, unit='elements whose bits differ')
    parity_report(test='infer_attention', kernel='run time of the file', seconds=round(time.time() - t0, 1))


def _lib_():
    from viewformer_amd import _lib
    return _lib.load()


@contextlib.contextmanager
def _register_staged():
    """vf_attn_blockcausal_bf16_v2 without the LDS-DMA kernel: the file under test is attention_lp.hip"""
    from viewformer_amd import _lib
    prev = _lib.select(_lib.SEL_ATTN_DMA, 0)
    try:
        yield
    finally:
        _lib.select(_lib.SEL_ATTN_DMA, prev)


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _close(key, got, want, mag, what):
    r = A.ratio(got.double().cpu(), want, mag, I.UNIT[key])
    _worst[key] = max(_worst.get(key, 0.0), r)
    print(f'{key} [{what}]: worst {r:.3g} units (c = {C[key]:g})')
    assert r <= C[key], f'{key} [{what}]: {r:.3g} x unit x magnitude exceeds c = {C[key]:g}'


def _same_bits(key, a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (key, what)
    it = torch.int32 if a.dtype == F32 else torch.int16
    bad = int((a.contiguous().view(it) != b.contiguous().view(it)).sum())
    _worst[key] = max(_worst.get(key, 0), bad)
    assert bad == 0, f'{key} [{what}]: {bad} elements differ in their bits'


def _new(shape, dt, dev):
    return torch.full(shape, NAN, dtype=dt, device=dev)


# ------------------------------------------------------------------ block-causal kernels
@functools.lru_cache(maxsize=None)
def _bref(arm, name):
    return I.bc_reference(I.BC_BY_NAME[name], arm)[1]


class Bufs:
    """operands and the NaN-filled output of one block-causal launch.  'fused': V | Q | K thirds of one [B*T][3d + pad] buffer; 'split':
    separate buffers whose leading dimensions all differ"""

    def __init__(self, case, qkv, in16, out16, dev, layout='fused'):
        name, B, H, T, L, spec, scale, kind = case
        self.case, self.in16, self.out16 = case, in16, out16
        d, M = H * 64, B * T
        dt, pad = (BF, 8) if in16 else (F32, 4)
        q, k, v = qkv
        if layout == 'fused':
            buf = _new((M, 3 * d + pad), dt, dev)
            self.v, self.q, self.k = buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:3 * d]
            self.wide = [(buf, 3 * d)]
        else:
            bq, bk, bv = _new((M, d + pad), dt, dev), _new((M, d + 2 * pad), dt, dev), _new((M, d + 3 * pad), dt, dev)
            self.q, self.k, self.v = bq[:, :d], bk[:, :d], bv[:, :d]
            self.wide = [(bq, d), (bk, d), (bv, d)]
        for dst, src in ((self.q, q), (self.k, k), (self.v, v)):
            dst.copy_(src.to(dev))
        bo = _new((M, d + 4), BF if out16 else F32, dev)
        self.out = bo[:, :d]
        self.wide.append((bo, d))

    def run(self, kernel, skip, spec=None):
        name, B, H, T, L, spec0, scale, kind = self.case
        spec = spec0 if spec is None else spec
        lds = [t.stride(0) for t in (self.q, self.k, self.v, self.out)]
        lib = _lib_()
        if kernel == 'x6':
            rc = lib.vf_attn_blockcausal_x6(_P(self.q), _P(self.k), _P(self.v), _P(self.out), B, H, T, L, *lds, scale, skip, spec, _strm())
        else:
            fn = lib.vf_attn_blockcausal_fp8 if kernel == 'fp8' else lib.vf_attn_blockcausal_bf16_v2
            rc = fn(_P(self.q), _P(self.k), _P(self.v), int(self.in16), _P(self.out), int(self.out16), B, H, T, L, *lds, scale, skip, spec, _strm())
        torch.cuda.synchronize()
        return rc

    def pads_untouched(self):
        return all(bool(torch.isnan(t[:, used:]).all()) for t, used in self.wide)


def _run_both(kernel, case, qkv, in16, out16, dev, layout, ref, what):
    """the dense and the skipping form of one (kernel, operands, dtype form): each against float64, then bit for bit against each other
    -> the skipping form's output"""
    outs = []
    for skip in (0, 1):
        b = Bufs(case, qkv, in16, out16, dev, layout)
        assert b.run(kernel, skip) == OK
        _close(kernel, b.out, *ref, f'{what} skip_masked {skip}')
        assert b.pads_untouched(), f'{what}: a padding column was written'
        outs.append(b.out)
    _same_bits(f'{kernel} skip_masked 1 = dense', outs[1], outs[0], what)
    return outs[1]


@pytest.mark.parametrize('name', [c[0] for c in I.BC_CASES])
def test_x6_against_fp64(dev, name):
    case = I.BC_BY_NAME[name]
    qkv = I.bc_inputs(case, 'x6')
    out = _run_both('x6', case, qkv, False, False, dev, 'fused', _bref('x6', name), name)
    if name == I.SPLIT_CASE:
        _same_bits('x6 split buffers = fused', _run_both('x6', case, qkv, False, False, dev, 'split', _bref('x6', name), name + ' split'), out, name)
    if name == 'T256 L64 twin4':                                                 # Vc >= nviews is plain block-causal
        p = Bufs(case, qkv, False, False, dev)
        assert p.run('x6', 1, spec=-1) == OK
        _same_bits('x6 twin Vc >= nviews = causal', p.out, out, name)


def _low_precision(kernel, dev, name):
    """lp and fp8 share a source and a test: the dtype forms on bf16-exact operands with the relations between them; lp also the raw form"""
    case = I.BC_BY_NAME[name]
    qkv = I.bc_inputs(case, kernel)
    ref = _bref(kernel, name)
    outs = {}
    for in16, out16 in I.lp_forms(name):
        outs[(in16, out16)] = _run_both(kernel, case, qkv, in16, out16, dev, 'fused', ref, f'{name} in_bf16 {in16} out_bf16 {out16}')
    if name == I.SPLIT_CASE:
        o = _run_both(kernel, case, qkv, 1, 0, dev, 'split', ref, f'{name} split')
        _same_bits(f'{kernel} split buffers = fused', o, outs[(1, 0)], name)
    if name in I.LP_ALL_FORMS:
        for in16 in (0, 1):
            assert torch.equal(outs[(in16, 1)], outs[(in16, 0)].to(BF)), f'{kernel} [{name}]: bf16 out is not the fp32 out rounded once (in_bf16 {in16})'
        for out16 in (0, 1):
            _same_bits(f'{kernel} bf16 in = fp32 in of the same values', outs[(1, out16)], outs[(0, out16)], name)
    if name == 'T256 L64 twin4':
        p = Bufs(case, qkv, 1, 0, dev)
        assert p.run(kernel, 1, spec=-1) == OK
        _same_bits(f'{kernel} twin Vc >= nviews = causal', p.out, outs[(1, 0)], name)
    if kernel == 'lp':                                                           # fp32 operands that are not bf16 numbers: the kernel rounds them
        raw = I.bc_inputs(case, 'x6')
        o32 = _run_both('lp', case, raw, 0, 0, dev, 'fused', _bref('x6', name), f'{name} raw fp32 in, fp32 out')
        o16 = _run_both('lp', case, raw, 0, 1, dev, 'fused', _bref('x6', name), f'{name} raw fp32 in, bf16 out')
        assert torch.equal(o16, o32.to(BF)), f'lp [{name}]: bf16 out is not the fp32 out rounded once (raw operands)'


@pytest.mark.parametrize('name', [c[0] for c in I.BC_CASES])
def test_lp_against_fp64(dev, name):
    with _register_staged():
        _low_precision('lp', dev, name)


@pytest.mark.parametrize('name', [c[0] for c in I.BC_CASES])
def test_fp8_against_fp64(dev, name):
    _low_precision('fp8', dev, name)


# ------------------------------------------------------------------ prefix kernels
@functools.lru_cache(maxsize=None)
def _pref(name, exact16):
    return I.prefix_reference(I.PREFIX_BY_NAME[name], exact16)


class Prefix:
    """the query views (V | Q | K thirds of one [B*N*L][3d + pad] buffer), the cache in the case's layout and the NaN-filled output"""

    def __init__(self, case, x, in16, out16, dev, layout=None):
        name, B, Cc, N, kind, layout0, lens = case
        layout = layout or layout0
        self.B, self.Cc, self.N, self.in16, self.out16, self.dev = B, Cc, N, in16, out16, dev
        dt, pad = (BF, 8) if in16 else (F32, 4)
        self.dt = dt
        rows_c = Cc * I.LV
        qkv = _new((B * N * I.LV, 3 * D + pad), dt, dev)
        self.v, self.q, self.k = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D]
        for dst, src in ((self.q, x['q']), (self.k, x['k']), (self.v, x['v'])):
            dst.copy_(src.to(dev))
        self.wide = [(qkv, 3 * D)]
        if layout in ('fused', 'stride'):                                        # the context's c_attn buffer: its Q third is never read and stays NaN
            extra = 8 if layout == 'stride' else 0
            ld = 3 * D + pad
            ctx = _new((B, rows_c + extra, ld), dt, dev)
            self.kp, self.vp = ctx[:, :rows_c, 2 * D:3 * D], ctx[:, :rows_c, :D]
            self.ldkp = self.ldvp = ld
            self.pstride = (rows_c + extra) * ld
        else:                                                                    # K/V-only: two buffers, ldkp != ldvp != ldq, one prefix_stride for both
            self.ldkp, self.ldvp = D + pad, D + 2 * pad
            self.pstride = rows_c * self.ldvp + 2 * pad
            kb, vb = _new((B * self.pstride,), dt, dev), _new((B * self.pstride,), dt, dev)
            self.kp = kb.as_strided((B, rows_c, D), (self.pstride, self.ldkp, 1))
            self.vp = vb.as_strided((B, rows_c, D), (self.pstride, self.ldvp, 1))
        self.kp.copy_(x['kp'].to(dev))
        self.vp.copy_(x['vp'].to(dev))
        self.new_out()

    def new_out(self):
        bo = _new((self.B * self.N * I.LV, D + 4), BF if self.out16 else F32, self.dev)
        self.out = bo[:, :D]
        self.wide = self.wide[:1] + [(bo, D)]

    def hide_cache_from(self, b, view):
        """NaN into every cache row of scene b at or beyond ``view``"""
        self.kp[b, view * I.LV:] = NAN
        self.vp[b, view * I.LV:] = NAN

    def run(self, arm, lens=None, C_=None, only=None):
        """arm 'prefix bf16' / 'prefix f32eq'; ``lens``: [B][N] -> the VAR entry; ``C_``: the capacity argument; ``only`` = (b, n): that view
        alone, as a launch of B = 1, N = 1 on the same buffers"""
        B, N, C_ = self.B, self.N, self.Cc if C_ is None else C_
        q, k, v, kp, vp, out = self.q, self.k, self.v, self.kp, self.vp, self.out
        if only is not None:
            b, n = only
            r = slice((b * N + n) * I.LV, (b * N + n + 1) * I.LV)
            q, k, v, out, kp, vp = q[r], k[r], v[r], out[r], kp[b:b + 1], vp[b:b + 1]
            lens = None if lens is None else [[lens[b][n]]]
            B, N = 1, 1
        lib = _lib_()
        ctx = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=self.dev).reshape(-1)
        geo = (B, I.PREFIX_H, C_, N, I.LV, I.DH, self.q.stride(0), self.k.stride(0), self.v.stride(0), self.ldkp, self.ldvp, self.pstride,
               self.out.stride(0))
        tail = (_strm(),) if ctx is None else (_P(ctx), _strm())
        if arm == 'prefix bf16':
            fn = lib.vf_attn_prefix_bf16 if ctx is None else lib.vf_attn_prefix_var_bf16
            rc = fn(_P(q), _P(k), _P(v), _P(kp), _P(vp), int(self.in16), _P(out), int(self.out16), *geo, *tail)
        else:
            assert not self.in16 and not self.out16
            fn = lib.vf_attn_prefix_f32eq if ctx is None else lib.vf_attn_prefix_var_f32eq
            rc = fn(_P(q), _P(k), _P(v), _P(kp), _P(vp), _P(out), *geo, *tail)
        torch.cuda.synchronize()
        return rc

    def pads_untouched(self):
        return all(bool(torch.isnan(t[:, used:]).all()) for t, used in self.wide)


PREFIX_FORMS = [('prefix bf16', True, 1, 1), ('prefix bf16', True, 1, 0), ('prefix bf16', True, 0, 1), ('prefix bf16', True, 0, 0),
                ('prefix bf16', False, 0, 0), ('prefix bf16', False, 0, 1), ('prefix f32eq', False, 0, 0)]        # (arm, exact operands, in_bf16, out_bf16)


def _hide_unread(p, lens):
    if lens is not None:
        for b, row in enumerate(lens):
            p.hide_cache_from(b, max(row))


@pytest.mark.parametrize('name', [c[0] for c in I.PREFIX_CASES])
def test_prefix_against_fp64(dev, name):
    """every dtype form of both arms against float64 (VAR cases: through the VAR entries, the cache rows no view reaches turned to NaN);
    bf16 out = the fp32 out rounded once, bf16 in = fp32 in of the same values"""
    case = I.PREFIX_BY_NAME[name]
    lens = case[6]
    outs = {}
    for arm, exact, in16, out16 in PREFIX_FORMS:
        p = Prefix(case, I.prefix_inputs(case, exact), in16, out16, dev)
        _hide_unread(p, lens)
        assert p.run(arm, lens=lens) == OK
        _close(arm, p.out, *_pref(name, exact), f'{name} {"exact" if exact else "raw"} in_bf16 {in16} out_bf16 {out16}')
        assert p.pads_untouched(), f'{name}: a padding column was written'
        outs[(arm, exact, in16, out16)] = p.out
    for exact, in16 in ((True, 1), (True, 0), (False, 0)):
        assert torch.equal(outs[('prefix bf16', exact, in16, 1)], outs[('prefix bf16', exact, in16, 0)].to(BF)), f'{name}: bf16 out is not the fp32 out rounded once'
    for out16 in (0, 1):
        _same_bits('prefix bf16: bf16 in = fp32 in of the same values', outs[('prefix bf16', True, 1, out16)], outs[('prefix bf16', True, 0, out16)], name)


@pytest.mark.parametrize('name', [c[0] for c in I.PREFIX_CASES if c[6] is None])
def test_prefix_equals_the_twin_mask_pass(dev, name):
    """the header's claim: vf_attn_prefix_bf16 gives the bits of the register-staged kernel, vf_attn_prefix_f32eq those of
    vf_attn_blockcausal_x6, run in twin mode (Vc = C) over the concatenated sequence of C + N views — in every dtype form, against the
    skipping and the dense form"""
    case = I.PREFIX_BY_NAME[name]
    _, B, Cc, N, kind, layout, lens = case
    T = (Cc + N) * I.LV
    seq_case = (name, B, I.PREFIX_H, T, I.LV, Cc, 1.0, kind)
    for arm, exact, in16, out16 in PREFIX_FORMS:
        x = I.prefix_inputs(case, exact)
        p = Prefix(case, x, in16, out16, dev)
        assert p.run(arm) == OK
        for skip in (1, 0):
            s = Bufs(seq_case, I.prefix_sequence(x, B, Cc, N), in16, out16, dev)
            if arm == 'prefix f32eq':
                assert s.run('x6', skip) == OK
            else:
                with _register_staged():
                    assert s.run('lp', skip) == OK
            own = s.out.reshape(B, T, D)[:, Cc * I.LV:].reshape(B * N * I.LV, D)
            _same_bits(f'{arm} = the twin-mask pass', p.out, own, f'{name} in_bf16 {in16} out_bf16 {out16} skip_masked {skip}')


@pytest.mark.parametrize('name', [c[0] for c in I.PREFIX_CASES if c[6] is not None])
def test_prefix_var_relations(dev, name):
    """VAR with all lengths C = the fixed entry; a VAR view of length c >= 1 = the fixed entry with C = c on the same buffers and
    prefix_stride; a VAR view does not depend on cache rows at or beyond its length (NaN there), nor on its neighbours (alone = in the batch)"""
    case = I.PREFIX_BY_NAME[name]
    _, B, Cc, N, kind, layout, lens = case
    for arm, in16, out16 in (('prefix bf16', 1, 1), ('prefix bf16', 0, 0), ('prefix f32eq', 0, 0)):
        x = I.prefix_inputs(case, arm == 'prefix bf16')
        what = f'{name} in_bf16 {in16} out_bf16 {out16}'
        p = Prefix(case, x, in16, out16, dev)
        assert p.run(arm) == OK
        fixed = p.out
        p.new_out()
        assert p.run(arm, lens=[[Cc] * N] * B) == OK
        _same_bits(f'{arm} VAR all lengths C = fixed', p.out, fixed, what)
        p.new_out()
        assert p.run(arm, lens=lens) == OK
        var = p.out
        for b in range(B):
            for n in range(N):
                c = lens[b][n]
                r = slice((b * N + n) * I.LV, (b * N + n + 1) * I.LV)
                h = Prefix(case, x, in16, out16, dev)
                h.hide_cache_from(b, c)
                assert h.run(arm, lens=lens) == OK
                _same_bits(f'{arm} VAR view ignores the cache beyond its length', h.out[r], var[r], f'{what} view ({b}, {n}) length {c}')
                h.new_out()
                assert h.run(arm, lens=lens, only=(b, n)) == OK
                _same_bits(f'{arm} VAR view alone = in its batch', h.out[r], var[r], f'{what} view ({b}, {n})')
                assert bool(torch.isnan(h.out[:r.start]).all()) and bool(torch.isnan(h.out[r.stop:]).all())
                if c >= 1:
                    f = Prefix(case, x, in16, out16, dev)
                    assert f.run(arm, C_=c) == OK
                    _same_bits(f'{arm} VAR length c = fixed with C = c', f.out[r], var[r], f'{what} view ({b}, {n}) length {c}')


@pytest.mark.parametrize('name', ['B2 C1 N5', 'B2 C2 N3', 'B1 C3 N4'])
def test_prefix_view_does_not_depend_on_N_or_its_position(dev, name):
    """each view alone (B = 1, N = 1, first in its launch) against the view in the full launch, whatever its group and slot"""
    case = I.PREFIX_BY_NAME[name]
    _, B, Cc, N, kind, layout, lens = case
    for arm, in16, out16 in (('prefix bf16', 1, 1), ('prefix bf16', 0, 0), ('prefix f32eq', 0, 0)):
        x = I.prefix_inputs(case, arm == 'prefix bf16')
        p = Prefix(case, x, in16, out16, dev)
        assert p.run(arm) == OK
        full = p.out
        p.new_out()
        for b in range(B):
            for n in range(N):
                assert p.run(arm, only=(b, n)) == OK
        _same_bits(f'{arm} view alone = in its batch', p.out, full, f'{name} in_bf16 {in16} out_bf16 {out16}')
        assert p.pads_untouched()


# ------------------------------------------------------------------ refusals
def test_prefix_refusals(dev):
    """every argument set below is refused by the entry's own checks before any launch (or is the documented no-op): the output keeps its NaN"""
    case = I.PREFIX_BY_NAME['B2 C2 N3']
    _, B, Cc, N, kind, layout, lens = case
    lib, s = _lib_(), _strm()
    H, w = I.PREFIX_H, I.PREFIX_H * 64
    for in16 in (1, 0):
        p = Prefix(case, I.prefix_inputs(case, True), in16, in16, dev)
        ctx = torch.full((B * N,), Cc, dtype=torch.int32, device=dev)
        ldq, ldo = p.q.stride(0), p.out.stride(0)

        def call(entry, B_=B, C_=Cc, N_=N, L_=64, dh_=64, ldq_=ldq, ldk_=ldq, ldv_=ldq, ldkp_=p.ldkp, ldvp_=p.ldvp, ps_=p.pstride, ldo_=ldo, ctx_=ctx, q_=p.q):
            geo = (B_, H, C_, N_, L_, dh_, ldq_, ldk_, ldv_, ldkp_, ldvp_, ps_, ldo_)
            if entry == 'bf16':
                return lib.vf_attn_prefix_bf16(_P(q_), _P(p.k), _P(p.v), _P(p.kp), _P(p.vp), in16, _P(p.out), in16, *geo, s)
            if entry == 'var_bf16':
                return lib.vf_attn_prefix_var_bf16(_P(q_), _P(p.k), _P(p.v), _P(p.kp), _P(p.vp), in16, _P(p.out), in16, *geo, _P(ctx_), s)
            if entry == 'f32eq':
                return lib.vf_attn_prefix_f32eq(_P(q_), _P(p.k), _P(p.v), _P(p.kp), _P(p.vp), _P(p.out), *geo, s)
            return lib.vf_attn_prefix_var_f32eq(_P(q_), _P(p.k), _P(p.v), _P(p.kp), _P(p.vp), _P(p.out), *geo, _P(ctx_), s)
        for entry in (('bf16', 'var_bf16') if in16 else ('bf16', 'var_bf16', 'f32eq', 'var_f32eq')):
            assert call(entry, L_=48) == UNSUPPORTED and call(entry, L_=128) == UNSUPPORTED, entry
            assert call(entry, dh_=32) == UNSUPPORTED and call(entry, dh_=128) == UNSUPPORTED, entry
            assert call(entry, C_=0) == UNSUPPORTED, entry
            assert call(entry, C_=-1) == BAD_ARG, entry                           # (a negative capacity is a bad argument, not an unsupported shape)
            assert call(entry, q_=None) == BAD_ARG, entry
            for ld in ('ldq_', 'ldk_', 'ldv_', 'ldkp_', 'ldvp_', 'ldo_'):
                assert call(entry, **{ld: w - 8}) == BAD_ARG, (entry, ld)
            is16 = in16 and entry in ('bf16', 'var_bf16')
            for ld in ('ldq_', 'ldk_', 'ldv_', 'ldkp_', 'ldvp_'):
                assert call(entry, **{ld: w + (4 if is16 else 2)}) == BAD_ARG, (entry, ld)     # % 8 (bf16) / % 4 (fp32) broken, still >= H * 64
            assert call(entry, ps_=p.pstride + (4 if is16 else 2)) == BAD_ARG, entry
            assert call(entry, ps_=-p.pstride) == BAD_ARG, entry
            assert call(entry, ldo_=ldo + 2) == BAD_ARG, entry
            if entry.startswith('var'):
                assert call(entry, ctx_=None) == BAD_ARG, entry
            assert call(entry, B_=0) == OK and call(entry, N_=0) == OK, entry
        torch.cuda.synchronize()
        assert bool(torch.isnan(p.out).all()) and p.pads_untouched()


def test_blockcausal_refusals(dev):
    case = I.BC_BY_NAME['T64 L64 causal s.125']
    _, B, H, T, L, spec, scale, kind = case
    lib, s = _lib_(), _strm()
    w = H * 64
    with _register_staged():
        for in16 in (1, 0):
            b = Bufs(case, I.bc_inputs(case, 'lp'), in16, in16, dev)
            ld, ldo = b.q.stride(0), b.out.stride(0)

            def low(fn, q_=b.q, out_=b.out, ldq_=ld, ldk_=ld, ldv_=ld, ldo_=ldo, scale_=scale, T_=T):
                return fn(_P(q_), _P(b.k), _P(b.v), in16, _P(out_), in16, B, H, T_, L, ldq_, ldk_, ldv_, ldo_, scale_, 1, spec, s)
            for fn in (lib.vf_attn_blockcausal_bf16_v2, lib.vf_attn_blockcausal_fp8):
                assert low(fn, scale_=0.0) == BAD_ARG and low(fn, scale_=-1.0) == BAD_ARG and low(fn, scale_=NAN) == BAD_ARG
                assert low(fn, q_=None) == BAD_ARG and low(fn, out_=None) == BAD_ARG and low(fn, T_=0) == BAD_ARG
                for ldn in ('ldq_', 'ldk_', 'ldv_', 'ldo_'):
                    assert low(fn, **{ldn: w - 8}) == BAD_ARG, ldn
                    assert low(fn, **{ldn: w + 2}) == BAD_ARG, ldn                # % 4 broken in either dtype
                if in16:
                    for ldn in ('ldq_', 'ldk_', 'ldv_'):
                        assert low(fn, **{ldn: w + 4}) == BAD_ARG, ldn            # bf16 rows are read as 16-byte vectors: % 8
            torch.cuda.synchronize()
            assert bool(torch.isnan(b.out).all())
    b = Bufs(case, I.bc_inputs(case, 'x6'), 0, 0, dev)
    ld, ldo = b.q.stride(0), b.out.stride(0)

    def x6(q_=b.q, ldq_=ld, ldk_=ld, ldv_=ld, ldo_=ldo, T_=T):
        return lib.vf_attn_blockcausal_x6(_P(q_), _P(b.k), _P(b.v), _P(b.out), B, H, T_, L, ldq_, ldk_, ldv_, ldo_, scale, 1, spec, s)
    assert x6(q_=None) == BAD_ARG and x6(T_=0) == BAD_ARG
    for ldn in ('ldq_', 'ldk_', 'ldv_', 'ldo_'):
        assert x6(**{ldn: w - 4}) == BAD_ARG and x6(**{ldn: w + 2}) == BAD_ARG, ldn
    torch.cuda.synchronize()
    assert bool(torch.isnan(b.out).all())
