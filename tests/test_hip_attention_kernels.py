"""GPU: the six entry points of the training attention one by one against the float64 references of tests/attention_kernels_ref.py (pinned
on the CPU by tests/test_attention_kernels_ref_host.py): vf_attn_blockcausal_lse_f32, vf_attn_bwd_prep_f32, vf_attn_bwd_f32 and
vf_attn_blockcausal_bf16_lse, vf_attn_bwd_prep_bf16, vf_attn_bwd_bf16, called through the C ABI.

Every output is judged on its own, element by element: |got - want| <= c x unit x magnitude, unit = 2^-24 for the f32 kernels and 2^-9 for
the bf16 kernels, the magnitude being the reference expression with every summand replaced by its absolute value plus the score term
described in attention_kernels_ref.py.  dq, dk and dv have a magnitude and a constant each: no norm over a joined buffer.  ``TABLE`` holds
one (basis, c) per kernel output: the basis is the worst error the CPU restatement of the kernel's formula shows against float64 on these
very inputs, as the host file measures and prints it, and c = 4 x basis rounded up to a power of two — never a figure taken from the
kernel.  Every measured worst ratio goes to the parity report (profiles/attention_kernels_parity.txt).

Outputs are pre-filled with NaN, operands are thirds of one [B*T][3d + pad] buffer (a second layout: separate buffers with different leading
dimensions) and the padding columns must still be NaN afterwards.  Every backward test feeds the kernel the REFERENCE's lse and D rounded
to float32, so that a forward error can neither hide nor cause a backward failure; one chained case per arm runs forward, prep and backward
as the trainer does.  Shapes are the smallest at which each path of the shape handling runs (attention_kernels_ref.py: F32_CASES,
BF16_CASES); the 64-view cases (the documented limit of the bf16 kernels' 64-bit view masks) take their float64 reference on the device."""
import ctypes

import numpy as np
import pytest
import torch

import attention_kernels_ref as A
import training_kernels_ref as R
from conftest import parity_report

pytestmark = pytest.mark.gpu

# kernel output: (basis, c).  basis = worst error of the CPU restatement against float64 over the cases, in units of 2^-24 (f32) or
# 2^-9 (bf16) x magnitude, as test_attention_kernels_ref_host.py measures and prints it; c = 4 x basis, rounded up to a power of two.
TABLE = {
    'f32 out': (1.71, 8.0),
    'f32 lse': (2.39, 16.0),
    'f32 D': (1.77, 8.0),
    'f32 dq': (0.300, 2.0),
    'f32 dk': (0.393, 2.0),
    'f32 dv': (2.07, 16.0),
    'bf16 out': (0.277, 2.0),
    'bf16 lse': (0.510, 4.0),
    'bf16 D': (1.89e-5, 2.0 ** -13),
    'bf16 dq': (0.0378, 0.25),
    'bf16 dk': (0.0398, 0.25),
    'bf16 dv': (0.221, 1.0),
}
BASIS = {k: b for k, (b, c) in TABLE.items()}
C = {k: c for k, (b, c) in TABLE.items()}

BAD_ARG, UNSUPPORTED = -1, -2
NAN = float('nan')
_worst = {}
_refs = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    _refs.clear()
    for k in sorted(_worst):
        parity_report(test='attention_kernels', kernel=k, worst_ratio=_worst[k], c=C.get(k, 0.0), basis=BASIS.get(k, 0.0),
                      unit=('2^-9 x magnitude' if k.startswith('bf16') else '2^-24 x magnitude') if k in C else 'mismatching elements')


def _lib_():
    from viewformer_amd import _lib
    return _lib.load()


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _close(key, got, want, mag, what):
    unit = A.U16 if key.startswith('bf16') else A.U32
    r = A.ratio(got.to(want.device), want, mag, unit)
    _worst[key] = max(_worst.get(key, 0.0), r)
    print(f'{key} [{what}]: worst {r:.3g} units (c = {C[key]:g})')
    assert r <= C[key], f'{key} [{what}]: {r:.3g} x unit x magnitude exceeds c = {C[key]:g}'


def _same_bits(key, a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    bad = int((a.contiguous().view(it) != b.contiguous().view(it)).sum())
    _worst[key] = max(_worst.get(key, 0), bad)
    assert bad == 0, f'{key} [{what}]: {bad} elements differ in their bits'


def _ref(case, bf16, dev):
    key = (case[0], bf16)
    if key not in _refs:
        _refs[key] = A.reference(case, bf16, device=dev)
    return _refs[key]


class Bufs:
    """the operands and NaN-filled outputs of one case on the device.  'fused': V | Q | K thirds of one [B*T][3d + pad] buffer, the gradients
    dV | dQ | dK thirds of another; 'split': separate buffers whose leading dimensions all differ"""

    def __init__(self, case, bf16, dev, layout='fused', grads_bf16=False, inputs=None):
        name, B, H, T, L, spec, scale, rate, kind = case
        self.case, self.bf16, self.d, self.M = case, bf16, H * 64, B * T
        d, M = self.d, self.M
        pad = 8 if bf16 else 4
        dt = torch.bfloat16 if bf16 else torch.float32
        gdt = torch.bfloat16 if grads_bf16 else torch.float32
        gpad = 8 if grads_bf16 else 4
        q, k, v, dout = inputs if inputs is not None else A.inputs(case, bf16)

        def new(cols, dtype=dt):
            return torch.full((M, cols), NAN, dtype=dtype, device=dev)
        if layout == 'fused':
            self.qkv = new(3 * d + pad)
            self.v, self.q, self.k = self.qkv[:, :d], self.qkv[:, d:2 * d], self.qkv[:, 2 * d:3 * d]
            self.g = new(3 * d + gpad, gdt)
            self.dv, self.dq, self.dk = self.g[:, :d], self.g[:, d:2 * d], self.g[:, 2 * d:3 * d]
            self.wide = [(self.qkv, 3 * d), (self.g, 3 * d)]
        else:
            bq, bk, bv = new(d + pad), new(d + 2 * pad), new(d + 3 * pad)
            gq, gk, gv = new(d + 3 * gpad, gdt), new(d + gpad, gdt), new(d + 2 * gpad, gdt)
            self.q, self.k, self.v, self.dq, self.dk, self.dv = bq[:, :d], bk[:, :d], bv[:, :d], gq[:, :d], gk[:, :d], gv[:, :d]
            self.wide = [(t, d) for t in (bq, bk, bv, gq, gk, gv)]
        self.q.copy_(q.to(dev))
        self.k.copy_(k.to(dev))
        self.v.copy_(v.to(dev))
        bo, bdo = new(d + 2 * pad), new(d + pad)
        self.out, self.dout = bo[:, :d], bdo[:, :d]
        self.dout.copy_(dout.to(dev))
        self.wide += [(bo, d), (bdo, d)]
        self.lse = torch.full((B, H, T), NAN, device=dev)
        self.D = torch.full((B, H, T), NAN, device=dev)

    def pads_untouched(self):
        return all(bool(torch.isnan(t[:, used:]).all()) for t, used in self.wide)

    def ld(self, t):
        return t.stride(0)

    # ---- the entry points through the C ABI
    def forward(self, skip_masked=1, rate=None, plane0=0, spec=None):
        name, B, H, T, L, spec0, scale, rate0, kind = self.case
        rate = rate0 if rate is None else rate
        spec = spec0 if spec is None else spec
        ld = self.ld
        if self.bf16:
            return _lib_().vf_attn_blockcausal_bf16_lse(_P(self.q), _P(self.k), _P(self.v), _P(self.out), _P(self.lse), B, H, T, L, ld(self.q), ld(self.k),
                                                        ld(self.v), ld(self.out), scale, spec, rate, A.SEED, A.SITE, plane0, _strm())
        return _lib_().vf_attn_blockcausal_lse_f32(_P(self.q), _P(self.k), _P(self.v), _P(self.out), _P(self.lse), B, H, T, L, ld(self.q), ld(self.k),
                                                   ld(self.v), ld(self.out), scale, skip_masked, spec, rate, A.SEED, A.SITE, plane0, _strm())

    def prep(self, out=None):
        name, B, H, T, *_ = self.case
        out = self.out if out is None else out
        fn = _lib_().vf_attn_bwd_prep_bf16 if self.bf16 else _lib_().vf_attn_bwd_prep_f32
        return fn(_P(self.dout), _P(out), _P(self.D), B, H, T, self.ld(self.dout), self.ld(out), _strm())

    def backward(self, lse, D, rate=None, plane0=0, spec=None, do_q=True, do_kv=True):
        name, B, H, T, L, spec0, scale, rate0, kind = self.case
        rate = rate0 if rate is None else rate
        spec = spec0 if spec is None else spec
        ld = self.ld
        if self.bf16:
            return _lib_().vf_attn_bwd_bf16(_P(self.q), _P(self.k), _P(self.v), _P(self.dout), _P(lse), _P(D), _P(self.dq) if do_q else None,
                                            _P(self.dk) if do_kv else None, _P(self.dv) if do_kv else None, 1 if self.dq.dtype == torch.bfloat16 else 0,
                                            B, H, T, L, ld(self.q), ld(self.k), ld(self.v), ld(self.dout), ld(self.dq), ld(self.dk), ld(self.dv), scale,
                                            spec, rate, A.SEED, A.SITE, plane0, _strm())
        return _lib_().vf_attn_bwd_f32(_P(self.q), _P(self.k), _P(self.v), _P(self.dout), _P(lse), _P(D), _P(self.dq), _P(self.dk), _P(self.dv), B, H, T, L,
                                       ld(self.q), ld(self.k), ld(self.v), ld(self.dout), ld(self.dq), ld(self.dk), ld(self.dv), scale, spec, rate,
                                       A.SEED, A.SITE, plane0, _strm())


def _arm(bf16):
    return 'bf16' if bf16 else 'f32'


def _check_forward(case, bf16, dev, layout):
    ref = _ref(case, bf16, dev)
    arm, what = _arm(bf16), f'{case[0]} {layout}'
    res = []
    for skip in ((1,) if bf16 else (0, 1)):
        b = Bufs(case, bf16, dev, layout)
        assert b.forward(skip_masked=skip) == 0
        torch.cuda.synchronize()
        _close(f'{arm} out', b.out.double(), *ref.out, f'{what} skip_masked {skip}')
        _close(f'{arm} lse', b.lse, *ref.lse, f'{what} skip_masked {skip}')
        assert b.pads_untouched(), f'{what}: a padding column was written'
        assert bool(torch.isnan(b.g).all() if layout == 'fused' else torch.isnan(b.dq).all())
        res.append(b)
    if len(res) == 2:                                                            # dense and tile-skipping forms: within the same bound of each other
        _close('f32 out', res[1].out.double(), res[0].out.double(), ref.out[1], f'{what} skip_masked 1 against 0')
        _close('f32 lse', res[1].lse, res[0].lse.double(), ref.lse[1], f'{what} skip_masked 1 against 0')
    return res[-1]


def _check_backward(case, bf16, dev, layout, b=None, lse=None, D=None, what=''):
    ref = _ref(case, bf16, dev)
    arm = _arm(bf16)
    what = f'{case[0]} {layout} {what}'
    b = Bufs(case, bf16, dev, layout) if b is None else b
    lse = ref.lse[0].float().contiguous() if lse is None else lse
    D = ref.D[0].float().contiguous() if D is None else D
    assert b.backward(lse, D) == 0
    torch.cuda.synchronize()
    for o in ('dq', 'dk', 'dv'):
        _close(f'{arm} {o}', getattr(b, o).double(), *getattr(ref, o), what)
    assert b.pads_untouched(), f'{what}: a padding column was written'
    return b


# ------------------------------------------------------------------ f32 kernels
@pytest.mark.parametrize('name', [c[0] for c in A.F32_CASES])
def test_f32_forward_with_lse(dev, name):
    """out and lse of the dense (skip_masked 0) and the tile-skipping (1) form against float64 and against each other; both layouts"""
    case = A.F32_BY_NAME[name]
    b = _check_forward(case, False, dev, 'fused')
    _check_forward(case, False, dev, 'split')
    if name == 'T256 L64 twin4':                                                 # Vc >= nviews is plain block-causal, bit for bit
        p = Bufs(case, False, dev)
        assert p.forward(spec=-1) == 0
        _same_bits('f32 twin Vc >= nviews = causal', p.out, b.out, name)
        _same_bits('f32 twin Vc >= nviews = causal', p.lse, b.lse, name)


@pytest.mark.parametrize('name', [c[0] for c in A.F32_CASES])
def test_f32_prep_row_sums(dev, name):
    """D = rowsum(dO O) on its own, from the reference's out rounded to float32, in both layouts"""
    case = A.F32_BY_NAME[name]
    _, B, H, T, *_ = case
    ref = _ref(case, False, dev)
    for layout in ('fused', 'split'):
        b = Bufs(case, False, dev, layout)
        b.out.copy_(ref.out[0].float())
        assert b.prep() == 0
        _close('f32 D', b.D, *A.rowsum_D(b.dout, b.out, B, H, T), f'{name} {layout}')
        assert b.pads_untouched()


@pytest.mark.parametrize('name', [c[0] for c in A.F32_CASES])
def test_f32_backward(dev, name):
    """dq, dk, dv each against float64, the backward fed the reference's lse and D; both layouts"""
    case = A.F32_BY_NAME[name]
    b = _check_backward(case, False, dev, 'fused')
    _check_backward(case, False, dev, 'split')
    if name == 'T256 L64 twin4':
        ref = _ref(case, False, dev)
        p = Bufs(case, False, dev)
        assert p.backward(ref.lse[0].float().contiguous(), ref.D[0].float().contiguous(), spec=-1) == 0
        _same_bits('f32 twin Vc >= nviews = causal', p.g[:, :3 * p.d], b.g[:, :3 * b.d], name)


@pytest.mark.parametrize('name', ['T576 L64 streams3x3 drop', 'T70 none drop'])
def test_f32_chain_as_the_trainer_runs_it(dev, name):
    case = A.F32_BY_NAME[name]
    b = _check_forward(case, False, dev, 'fused')
    assert b.prep() == 0
    _check_backward(case, False, dev, 'fused', b=b, lse=b.lse, D=b.D, what='chained')


def test_f32_refusals(dev):
    """bad arguments are refused before any launch: the outputs keep their NaN"""
    case = A.F32_BY_NAME['T64 L64 causal s.125']
    _, B, H, T, L, spec, scale, rate, kind = case
    b = Bufs(case, False, dev)
    lib, s = _lib_(), _strm()
    ld, ldo, w = b.ld(b.q), b.ld(b.out), H * 64
    lse, D = torch.zeros((B, H, T), device=dev), torch.zeros((B, H, T), device=dev)

    def fwd(q=b.q, out=b.out, ldq=ld, ldo_=ldo, rate_=0.0):
        return lib.vf_attn_blockcausal_lse_f32(_P(q), _P(b.k), _P(b.v), _P(out), _P(b.lse), B, H, T, L, ldq, ld, ld, ldo_, scale, 1, spec, rate_, 1, 1, 0, s)

    def bwd(q=b.q, dq=b.dq, ldq=ld, lddq=b.ld(b.dq), rate_=0.0):
        return lib.vf_attn_bwd_f32(_P(q), _P(b.k), _P(b.v), _P(b.dout), _P(lse), _P(D), _P(dq), _P(b.dk), _P(b.dv), B, H, T, L, ldq, ld, ld, b.ld(b.dout),
                                   lddq, b.ld(b.dk), b.ld(b.dv), scale, spec, rate_, 1, 1, 0, s)
    for f in (fwd, bwd):
        assert f(q=None) == BAD_ARG
        assert f(ldq=w - 4) == BAD_ARG
        assert f(ldq=ld + 2) == BAD_ARG
        assert f(rate_=1.0) == BAD_ARG
    assert fwd(out=None) == BAD_ARG and fwd(ldo_=ldo + 1) == BAD_ARG and bwd(dq=None) == BAD_ARG and bwd(lddq=w - 4) == BAD_ARG
    assert lib.vf_attn_bwd_prep_f32(None, _P(b.out), _P(b.D), B, H, T, b.ld(b.dout), ldo, s) == BAD_ARG
    assert lib.vf_attn_bwd_prep_f32(_P(b.dout), _P(b.out), _P(b.D), B, H, T, w - 4, ldo, s) == BAD_ARG
    assert lib.vf_attn_bwd_prep_f32(_P(b.dout), _P(b.out), _P(b.D), B, H, T, b.ld(b.dout), ldo + 2, s) == BAD_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (b.out, b.lse, b.D, b.g))


# ------------------------------------------------------------------ bf16 kernels
@pytest.mark.parametrize('name', [c[0] for c in A.BF16_CASES])
def test_bf16_forward_with_lse(dev, name):
    case = A.BF16_BY_NAME[name]
    b = _check_forward(case, True, dev, 'fused')
    if case[3] < A.BIG_T:
        _check_forward(case, True, dev, 'split')
    if name == '5 views twin9':
        p = Bufs(case, True, dev)
        assert p.forward(spec=-1) == 0
        _same_bits('bf16 twin Vc >= nviews = causal', p.out, b.out, name)
        _same_bits('bf16 twin Vc >= nviews = causal', p.lse, b.lse, name)


def test_bf16_forward_rounds_the_folded_q(dev):
    """the forward's q' = bf16(q scale log2 e) is what the dQ kernel re-materialises P from (attention_train_bf16.hip: FOLD), and a forward
    without that rounding is CLOSER to float64, so the comparison above cannot see it go.  This one is two-sided: at the large-score case the
    kernel's lse must lie by the restatement with the rounding and away from the restatement without it.  d = the two restatements'
    distance (CPU, in the units of the lse comparison).  Kernel and rounded restatement share every stated rounding and differ by float32
    summation order, 2^-24 against the 2^-9 that d is made of: d / 16 leaves that four thousand times its size; a kernel that skipped the
    rounding would sit at d from the first and at 0 from the second."""
    case = A.BF16_BY_NAME['4 views causal large']
    name, B, H, T, L, spec, scale, rate, kind = case
    q, k, v, dout = A.inputs(case, True)
    mag = _ref(case, True, dev).lse[1].cpu()
    _, lse_r = A.fwd_bf16(q, k, v, B, H, T, spec, scale)
    _, lse_u = A.fwd_bf16(q, k, v, B, H, T, spec, scale, unrounded_q=True)
    b = Bufs(case, True, dev)
    assert b.forward() == 0
    got = b.lse.cpu()
    d = A.ratio(lse_r, lse_u.double(), mag, A.U16)
    d_r, d_u = A.ratio(got, lse_r.double(), mag, A.U16), A.ratio(got, lse_u.double(), mag, A.U16)
    print(f'bf16 lse at large scores: restatements {d:.3g} units apart; kernel {d_r:.3g} from the rounded one, {d_u:.3g} from the un-rounded one')
    _worst['bf16 lse from the rounded restatement / distance of the two'] = d_r / d
    assert d > 0.1, d
    assert d_r <= d / 16 and d_u >= d / 2, (d, d_r, d_u)


@pytest.mark.parametrize('name', [c[0] for c in A.BF16_CASES])
def test_bf16_prep_row_sums(dev, name):
    case = A.BF16_BY_NAME[name]
    _, B, H, T, *_ = case
    ref = _ref(case, True, dev)
    for layout in ('fused', 'split'):
        b = Bufs(case, True, dev, layout)
        b.out.copy_(ref.out[0].float())                                          # (rounds to bf16)
        assert b.prep() == 0
        _close('bf16 D', b.D, *A.rowsum_D(b.dout, b.out, B, H, T), f'{name} {layout}')
        assert b.pads_untouched()


@pytest.mark.parametrize('name', [c[0] for c in A.BF16_CASES])
def test_bf16_backward(dev, name):
    """fp32 gradients against float64; bf16 gradients = the fp32 gradients rounded once; dq alone and dk / dv alone = the joint call, bit
    for bit"""
    case = A.BF16_BY_NAME[name]
    ref = _ref(case, True, dev)
    lse, D = ref.lse[0].float().contiguous(), ref.D[0].float().contiguous()
    b = _check_backward(case, True, dev, 'fused')
    if case[3] < A.BIG_T:
        _check_backward(case, True, dev, 'split')
    h = Bufs(case, True, dev, 'fused', grads_bf16=True)
    assert h.backward(lse, D) == 0
    for o in ('dq', 'dk', 'dv'):
        assert torch.equal(getattr(h, o), getattr(b, o).to(torch.bfloat16)), f'{name}: bf16 {o} is not the fp32 {o} rounded once'
    assert h.pads_untouched()
    for do_q in (True, False):
        p = Bufs(case, True, dev, 'fused')
        assert p.backward(lse, D, do_q=do_q, do_kv=not do_q) == 0
        if do_q:
            _same_bits('bf16 dq alone = joint', p.dq, b.dq, name)
            assert bool(torch.isnan(p.dk).all()) and bool(torch.isnan(p.dv).all())
        else:
            _same_bits('bf16 dk dv alone = joint', p.dk, b.dk, name)
            _same_bits('bf16 dk dv alone = joint', p.dv, b.dv, name)
            assert bool(torch.isnan(p.dq).all())
        assert p.pads_untouched()
    if name == '5 views twin9':
        p = Bufs(case, True, dev)
        assert p.backward(lse, D, spec=-1) == 0
        _same_bits('bf16 twin Vc >= nviews = causal', p.g[:, :3 * p.d], b.g[:, :3 * b.d], name)


@pytest.mark.parametrize('name', ['9 views streams3x3 drop', '4 views causal large'])
def test_bf16_chain_as_the_trainer_runs_it(dev, name):
    case = A.BF16_BY_NAME[name]
    b = _check_forward(case, True, dev, 'fused')
    assert b.prep() == 0
    _check_backward(case, True, dev, 'fused', b=b, lse=b.lse, D=b.D, what='chained')


def test_bf16_refusals(dev):
    case = A.BF16_BY_NAME['2 views causal s.125']
    _, B, H, T, L, spec, scale, rate, kind = case
    b = Bufs(case, True, dev)
    lib, s = _lib_(), _strm()
    ld, ldo = b.ld(b.q), b.ld(b.out)
    lse, D = torch.zeros((B, H, 65 * 64), device=dev), torch.zeros((B, H, 65 * 64), device=dev)

    def fwd(q=_P(b.q), T_=T, L_=L, ldq=ld, scale_=scale):
        return lib.vf_attn_blockcausal_bf16_lse(q, _P(b.k), _P(b.v), _P(b.out), _P(b.lse), B, H, T_, L_, ldq, ld, ld, ldo, scale_, spec, 0.0, 1, 1, 0, s)

    def bwd(q=_P(b.q), T_=T, L_=L, ldq=ld, scale_=scale):
        return lib.vf_attn_bwd_bf16(q, _P(b.k), _P(b.v), _P(b.dout), _P(lse), _P(D), _P(b.dq), _P(b.dk), _P(b.dv), 0, B, H, T_, L_, ldq, ld, ld,
                                    b.ld(b.dout), b.ld(b.dq), b.ld(b.dk), b.ld(b.dv), scale_, spec, 0.0, 1, 1, 0, s)
    # (more than 64 views: the backward's 64-bit view masks end there; the forward is the inference kernel, which walks every key view of a
    # longer sequence instead, so that call is not a refusal and is not made on these buffers)
    assert bwd(T_=65 * 64) == UNSUPPORTED
    for f in (fwd, bwd):
        assert f(L_=48) == UNSUPPORTED
        assert f(q=ctypes.c_void_p(b.q.data_ptr() + 8)) == UNSUPPORTED         # a pointer that is not 16-byte aligned
        assert f(ldq=ld + 4) in (BAD_ARG, UNSUPPORTED)                          # ld % 8 != 0
        assert f(scale_=0.0) == BAD_ARG and f(scale_=-1.0) == BAD_ARG
        assert f(q=None) == BAD_ARG
    assert lib.vf_attn_bwd_prep_bf16(_P(b.dout), _P(b.out), _P(b.D), B, H, T, b.ld(b.dout) + 4, ldo, s) == BAD_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (b.out, b.lse, b.D, b.g))


# ------------------------------------------------------------------ both arms
def _scene(x, B, T, i):
    return x.reshape(B, T, -1)[i]


@pytest.mark.parametrize('bf16', [False, True])
def test_drop_plane0_draws_the_masks_of_the_concatenated_batch(dev, bf16):
    """a batch of two scenes with plane 0 against the second scene alone with drop_plane0 = H: bit-identical out, lse and gradients"""
    case = (A.BF16_BY_NAME['9 views streams3x3 drop'] if bf16 else A.F32_BY_NAME['T70 none drop'])
    name, B, H, T, L, spec, scale, rate, kind = case
    assert B == 2 and rate > 0
    both = Bufs(case, bf16, dev)
    assert both.forward() == 0 and both.prep() == 0 and both.backward(both.lse, both.D) == 0
    one_case = (name, 1, H, T, L, spec, scale, rate, kind)
    second = tuple(_scene(x, B, T, 1).contiguous() for x in A.inputs(case, bf16))
    for plane0, same in ((H, True), (0, False)):
        one = Bufs(one_case, bf16, dev, inputs=second)
        assert one.forward(plane0=plane0) == 0 and one.prep() == 0 and one.backward(one.lse, one.D, plane0=plane0) == 0
        torch.cuda.synchronize()
        if same:
            key = f'{_arm(bf16)} drop_plane0'
            _same_bits(key, one.out, _scene(both.out, B, T, 1), 'out')
            _same_bits(key, one.lse[0], both.lse[1], 'lse')
            for o in ('dq', 'dk', 'dv'):
                _same_bits(key, getattr(one, o), _scene(getattr(both, o), B, T, 1), o)
        else:                                                                    # (the argument is not ignored)
            assert not torch.equal(one.out, _scene(both.out, B, T, 1))
            assert not torch.equal(one.dv, _scene(both.dv, B, T, 1))


@pytest.mark.parametrize('bf16', [False, True])
def test_dropout_leaves_the_log_sum_exp_alone(dev, bf16):
    """the same inputs with rate 0 and rate 0.2: lse is over the undropped weights, bit for bit"""
    case = (A.BF16_BY_NAME['9 views streams3x3 drop'] if bf16 else A.F32_BY_NAME['T70 none drop'])
    a, b = Bufs(case, bf16, dev), Bufs(case, bf16, dev)
    assert a.forward(rate=0.0) == 0 and b.forward(rate=0.2) == 0
    torch.cuda.synchronize()
    _same_bits(f'{_arm(bf16)} lse with / without dropout', a.lse, b.lse, case[0])
    assert not torch.equal(a.out, b.out)
