"""GPU: the bf16 GEMM family one by one against the float64 references of tests/gemm_kernels_ref.py (pinned on the CPU by
tests/test_gemm_kernels_ref_host.py): vf_gemm_bf16's staged 128-tile kernel, its direct 128-tile kernel in all four <bf16 in, bf16 out>
instantiations, the 256-tile kernel with every epilogue form it has, its tail tiles, the batched split-K form, the weight-gradient GEMM
vf_gemm_tn_bf16 through the C ABI with the test's own split counts, the slab fold vf_sum_slabs_f32 and the bf16 packings.

Exact class (selector inputs, dyadic inputs, the slab fold, the packings): the result must equal the reference as values, element for
element (R.mismatches == 0); a bf16 output must equal bf16_rne(want).  Rounded class, float32 output: |got - want| <= c x 2^-24 x
magnitude per element (R.worst_ratio).  Rounded class, bf16 output: the interval rule, bf16_rne(want - b) <= got <= bf16_rne(want + b)
with b that float32 bound — no relative 2^-8 allowance, which would hide truncation and a second rounding; no element is excluded.
``TABLE`` holds one (basis, c) per kernel class and epilogue function: the basis is the worst error the float32 CPU restatement of the
kernel's order shows against float64 on these very inputs, as the host file measures and prints it, and c = 4 x basis rounded up to a
power of two (the factor covers another valid summation order inside a matrix instruction, fused multiply-adds and the device's exp2 /
rcp) — never a figure taken from the kernel.  Every kernel's measured worst ratio goes to the parity report
(profiles/gemm_kernels_parity.txt).

Padding is poison: every operand passed with ld > its width carries NaN in its padding columns, every output is pre-filled with a
sentinel; the padding must keep it and the result must hold neither.  Inputs are built on the CPU from the reference module; nothing is
compared against another GPU kernel except where two kernels are BOTH held to float64 (VF_SEL_GEMM_G256 = 0) and where the packings'
bit-identity is the claim."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_kernels_ref as G
import training_kernels_ref as R
from conftest import parity_report

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16

# kernel class [+ epilogue function]: (basis, c).  basis = worst error of the float32 CPU restatement against float64 in units of
# 2^-24 x magnitude, as test_gemm_kernels_ref_host.py measures and prints it; c = 4 x basis, rounded up to a power of two.  The function
# classes carry the erf approximation's stated error inside their magnitude (G.FN_TERM).  A bf16 output is judged by the interval rule
# with the same constant.
TABLE = {
    'staged': (1.54, 8.0),
    'staged gelu': (1.42, 8.0),
    'splitk': (0.85, 4.0),
    'direct': (1.39, 8.0),
    'direct gelu': (1.23, 8.0),
    'direct gelu_bwd': (1.12, 8.0),
    'g256': (1.66, 8.0),
    'g256 gelu': (1.30, 8.0),
    'g256 gelu_grad': (1.02, 8.0),
    'g256 gelu_bwd': (1.29, 8.0),
    'g256 drop': (2.37, 16.0),
    'tail': (1.76, 8.0),
    'tail gelu': (1.53, 8.0),
    'tail drop': (2.27, 16.0),
    'tn dW': (1.50, 8.0),
    'tn db': (1.05, 8.0),
}
BASIS = {k: b for k, (b, c) in TABLE.items()}
C = {k: c for k, (b, c) in TABLE.items()}

EPI = {None: 0, 'gelu': 1, 'gelu_bwd': 2, 'dual': 3}
_worst = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        kc = k[:-5] if k.endswith(' bf16') else k
        rounded = kc in C and not k.endswith(' bf16')
        parity_report(test='gemm_kernels', kernel=k, worst_ratio=_worst[k], c=C.get(kc, 0.0), basis=BASIS.get(kc, 0.0),
                      unit='2^-24 x magnitude' if rounded else 'elements outside the interval of c' if kc in C else 'mismatching elements')


def _lib_():
    from viewformer_amd import _lib
    return _lib.load()


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _exact(kernel, got, want, what=''):
    want = torch.as_tensor(want)
    bad = R.mismatches(got.to(want.device) if torch.is_tensor(got) else got, want)
    _worst[kernel] = max(_worst.get(kernel, 0), bad)
    assert bad == 0, f'{kernel} {what}: {bad} elements differ from the reference'


def _close(kernel, got, want, mag, what='', c=None):
    c = C[kernel] if c is None else c
    r = R.worst_ratio(got.to(R.t64(want).device), want, mag)
    _worst[kernel] = max(_worst.get(kernel, 0.0), r)
    print(f'{kernel} {what}: worst {r:.3f} x 2^-24 x magnitude (c = {c:g})')
    assert r <= c, f'{kernel} {what}: {r:.3f} x 2^-24 x magnitude exceeds c = {c:g}'


def _same_bits(kernel, a, b, what=''):
    """two float32 or two bf16 tensors, bit for bit"""
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    assert a.dtype == b.dtype and a.shape == b.shape
    bad = int((a.contiguous().view(it) != b.contiguous().view(it)).sum())
    _worst[kernel] = max(_worst.get(kernel, 0), bad)
    assert bad == 0, f'{kernel} {what}: {bad} elements differ in their bits'


def _interval(kernel, got16, want, mag, what=''):
    """the interval rule for a bf16 output, with the float32 bound of the kernel's constant"""
    assert got16.dtype == BF16
    bad = G.interval_violations(got16, want, G.bound(mag, C[kernel]))
    _worst[kernel + ' bf16'] = max(_worst.get(kernel + ' bf16', 0), bad)
    print(f'{kernel} bf16 {what}: {bad} elements outside [bf16(want - b), bf16(want + b)], b = {C[kernel]:g} x 2^-24 x magnitude')
    assert bad == 0, f'{kernel} bf16 {what}: {bad} elements outside the interval of c = {C[kernel]:g}'


# ------------------------------------------------------------------ padding is poison
def _operand(t, pad, dev):
    """[M][W] -> the device tensor [M][W + pad] with NaN in the padding columns"""
    if not pad:
        return t.contiguous().to(dev)
    buf = torch.full((t.shape[0], t.shape[1] + pad), float('nan'), dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(dev)


def _outbuf(M, N, pad, dtype, dev):
    return torch.full((M, N + pad), G.SENTINEL, dtype=dtype, device=dev)


def _result(out, N, what):
    """the [M][N] result on the CPU: its padding untouched, no NaN and no sentinel left in it"""
    body, pad = out[:, :N], out[:, N:]
    assert bool((pad == G.SENTINEL).all()), f'{what}: the padding of an output row was written'
    assert not bool(torch.isnan(body).any()), f'{what}: NaN in the result (a padding column was read)'
    assert not bool((body == G.SENTINEL).any()), f'{what}: an element was not written'
    return body.cpu()


def _pack(W, dev):
    from viewformer_amd import ops
    return ops.pack_dense_kn_bf16(W.to(dev))


def _launch(dev, inp, wp, form, a16, o16, pads=(0, 0, 0), drop=None, keep=False):
    """one vf_gemm_bf16 launch of a form -> {'out': [M][N] on the CPU[, 'aux': ...]} (``keep``: the device buffers instead, unchecked)"""
    from viewformer_amd import ops
    f = G.FORMS[form]
    (M, K), N = inp['x'].shape, inp['W'].shape[1]
    pa, pc, pr = pads
    x = _operand(inp['x'].to(BF16) if a16 else inp['x'], pa, dev)
    out = _outbuf(M, N, pc, BF16 if o16 else F32, dev)
    aux = _outbuf(M, N, pc, BF16, dev) if f.get('epi') == 'dual' else None
    res = None
    if f.get('epi') == 'gelu_bwd':
        res = _operand(inp['g16'] if f.get('gelu_grad') else inp['u'].to(BF16) if f.get('res16') else inp['u'], pr, dev)
    elif f.get('res'):
        res = _operand(inp['res'], pr, dev)
    ops.igemm(x, wp, M, K, N, out, bias=inp['bias'].to(dev) if f.get('bias') else None, res=res, epilogue=EPI[f.get('epi')],
              lda=K + pa, ldc=N + pc, ldr=N + pr, bf16=True, a16=a16, o16=o16, out_aux=aux, res16=bool(f.get('res16')),
              gelu_grad=bool(f.get('gelu_grad')), drop=(drop[0], G.DROP_SEED, G.DROP_SITE, drop[1]) if f.get('drop') else None)
    if keep:
        return {'out': out, 'aux': aux}
    what = f'{form} ({M},{K},{N}) a16 {a16} o16 {o16} pads {pads}'
    got = {'out': _result(out, N, what)}
    if aux is not None:
        got['aux'] = _result(aux, N, what + ' aux')
    return got


def _judge(kernel, form, got, want, exact, what):
    """every output of a form against its reference: exactly (a bf16 output against bf16_rne(want)), by the float32 rule, or by the
    interval rule.  The GELU beside an exact pre-activation (dual on dyadic inputs) stays in the rounded class"""
    for name, (w, m) in want.items():
        g, fn = got[name], G.fn_class(form, name)
        key = kernel + (' ' + fn if fn else '')
        if exact and fn in ('', 'drop'):
            _exact(kernel + ' exact', g.float(), G.bf16_rne(w) if g.dtype == BF16 else w, f'{what} {name}')
        elif g.dtype == BF16:
            _interval(key, g, w, m, f'{what} {name}')
        else:
            _close(key, g, w, m, f'{what} {name}')


def _forward_case(dev, kernel, M, K, N, cls, runs, rows=None):
    """``runs`` = [(form, a16, o16, pads, drop)] on one input set: the float64 product is formed once"""
    inp = G.forward_inputs(M, K, N, cls)
    wp = _pack(inp['W'], dev)
    pre0, mag0 = G.gemm(inp['x'], inp['W'])
    for form, a16, o16, pads, drop in runs:
        got = _launch(dev, inp, wp, form, a16, o16, pads, drop)
        _judge(kernel, form, got, G.wants(form, inp, pre0, mag0, drop=drop), cls == 'dyadic',
               f'({M},{K},{N}) {cls} {form} a16 {a16} o16 {o16} pads {pads} drop {drop}')


EXACT_FORMS = ('none', 'bias', 'res', 'dual', 'gelu_bwd16_grad')      # the forms whose `out` is exact on dyadic inputs


# ------------------------------------------------------------------ selector inputs: every (k, n) of the packing, every row of x
def _selector_case(dev, kernel, K, N, a16, pads=(0, 0, 0)):
    """x [K][K] with one 1 per row at column pi(m): the result is bf16_rne(W)[pi] — plus the bias and then the residual, one float32
    rounding each, which the reference forms in float32 as the header orders them"""
    x, pi = G.selector(K, 600 + K + N)
    inp = dict(x=x, W=R.normal((K, N), 601 + K + N, 0.05), bias=R.normal((N,), 602 + N), res=R.normal((K, N), 603 + K + N))
    wp = _pack(inp['W'], dev)
    sel = G.bf16_rne(inp['W'])[pi].float()
    what = f'selector ({K},{K},{N}) a16 {a16} pads {pads}'
    _exact(kernel + ' exact', _launch(dev, inp, wp, 'none', a16, False, pads)['out'], sel, what)
    _exact(kernel + ' exact', _launch(dev, inp, wp, 'bias', a16, False, pads)['out'], sel + inp['bias'], what + ' bias')
    _exact(kernel + ' exact', _launch(dev, inp, wp, 'res', a16, False, pads)['out'], (sel + inp['bias']) + inp['res'], what + ' res')
    if K % 128 == 0:
        _exact(kernel + ' exact', _launch(dev, inp, wp, 'bias', a16, True, pads)['out'].float(), G.bf16_rne(sel + inp['bias']), what + ' bf16')


@pytest.mark.parametrize('K', G.STAGED_K)
def test_staged_kernel_selects(dev, K):
    for N in G.STAGED_N:
        for pa, _, pc, pr in G.PADS:
            _selector_case(dev, 'staged', K, N, False, (pa, pc, pr))


@pytest.mark.parametrize('K', G.DIRECT_K)
def test_direct_kernel_selects(dev, K):
    """M = K = 128 and 384 (three row tiles); bf16 x stays below the 256-tile kernel's shapes by N"""
    for N in (64, 129, 130, 256):
        for a16 in (False, True):
            if a16 and K >= 256 and N % 256 == 0:
                continue
            for pa, pa16, pc, pr in G.PADS:
                _selector_case(dev, 'direct', K, N, a16, (pa16 if a16 else pa, pc, pr))


@pytest.mark.parametrize('N', G.G256_N)
def test_g256_kernel_selects(dev, N):
    """M = K = 384: one full tile and a ragged one of 128 rows, six 64-deep stages"""
    for pa, pc, pr, _ in G.G256_PADS:
        _selector_case(dev, 'g256', 384, N, True, (pa, pc, pr))


# ------------------------------------------------------------------ the staged kernel
@pytest.mark.parametrize('K', G.STAGED_K)
@pytest.mark.parametrize('M', G.STAGED_M)
def test_staged_kernel(dev, M, K):
    """float32 x with K = 64 (one stage: the loop's only iteration re-stores its own stage) and 192 (three); one row, either side of the
    128-row tile, a ragged third tile; N ragged in its first and in its second column block; with and without padding in x, out and res"""
    for N in G.STAGED_N:
        for cls in ('dyadic', 'normal'):
            runs = [(form, False, False, (pa, pc, pr), None) for form in G.STAGED_FORMS for pa, _, pc, pr in G.PADS
                    if cls == 'normal' or form in EXACT_FORMS]
            _forward_case(dev, 'staged', M, K, N, cls, runs)


@pytest.mark.parametrize('M,N', G.STAGED_BATCHED)
def test_staged_kernel_batched_and_the_fold(dev, M, N):
    """ops.gemm_bf16_splitk's launch (batch 3 over K = 192: one 64-deep chunk per entry, x columns and packed chunks by stride) slab by
    slab, then the wrapper's folded result with accumulate on and off"""
    from viewformer_amd import ops
    K, S = 192, 3
    for cls in ('dyadic', 'normal'):
        inp = G.forward_inputs(M, K, N, cls, saved=False)
        wp = _pack(inp['W'], dev)
        parts = G.splitk(inp['x'], inp['W'], S)
        xd = inp['x'].to(dev)
        slabs = torch.full((S, M, N), G.SENTINEL, device=dev)
        ops.igemm(xd, wp, M, K // S, N, slabs, lda=K, bf16=True, batch=S, stride_x=K // S, stride_w=((N + 127) // 128) * 64 * 128,
                  stride_out=M * N)
        for s in range(S):
            got = _result(slabs[s], N, f'batched slab {s}')
            if cls == 'dyadic':
                _exact('staged exact', got, parts[s][0], f'({M},{K},{N}) slab {s}')
            else:
                _close('staged', got, *parts[s], f'({M},{K},{N}) batched slab {s}')
        for acc in (False, True):
            dst = inp['res'].to(dev).clone()
            ops.gemm_bf16_splitk(xd, wp, M, K, N, dst, S, accumulate=acc)
            w, m = G.fold([p[0] for p in parts], [p[1] for p in parts], inp['res'] if acc else None)
            if cls == 'dyadic':
                _exact('splitk exact', dst.cpu(), w, f'({M},{K},{N}) accumulate {acc}')
            else:
                _close('splitk', dst.cpu(), w, m, f'({M},{K},{N}) accumulate {acc}')


# ------------------------------------------------------------------ the direct kernel
@pytest.mark.parametrize('K', G.DIRECT_K)
@pytest.mark.parametrize('a16,o16', [(False, False), (True, False), (False, True), (True, True)])
def test_direct_kernel(dev, a16, o16, K):
    """all four instantiations below the 256-tile kernel's floor and at M = 300 with N no multiple of 256; N = 129 (an odd width: the
    scalar bf16 store), N = 130 with ldc 131 (scalar by the odd ldc) and ldc 132 (paired stores, a ragged block of two columns)"""
    for M, N in G.DIRECT_MN:
        for cls in ('dyadic', 'normal'):
            runs = []
            for form in G.DIRECT_FORMS[o16]:
                if cls == 'dyadic' and form not in EXACT_FORMS:
                    continue
                for i, ldc in enumerate(G.direct_ldc(N)):
                    pa, pa16, _, pr = G.PADS[min(i, 1)]
                    runs.append((form, a16, o16, (pa16 if a16 else pa, ldc - N, pr), None))
            _forward_case(dev, 'direct', M, K, N, cls, runs)


# ------------------------------------------------------------------ the 256-tile kernel
@pytest.mark.parametrize('K', G.G256_K)
@pytest.mark.parametrize('M', G.G256_M)
def test_g256_kernel(dev, M, K):
    """one tile; one row, 255 rows and 128 rows in a second tile; two and six stages; one and two column tiles; every form of the float32
    and of the bf16 epilogue; padded and unpadded operands (ldc and the bf16 ldr even, as the paired stores and loads need)"""
    for N in G.G256_N:
        for cls in ('dyadic', 'normal'):
            runs = [(form, True, o16, (pa, pc, pr16 if G.FORMS[form].get('res16') else pr), None)
                    for o16 in (False, True) for form in G.G256_FORMS[o16] for pa, pc, pr, pr16 in G.G256_PADS
                    if cls == 'normal' or form in EXACT_FORMS]
            _forward_case(dev, 'g256', M, K, N, cls, runs)


@pytest.mark.parametrize('K', G.G256_K)
@pytest.mark.parametrize('M', G.G256_M)
def test_g256_kernel_dropout(dev, M, K):
    """the fused output dropout: rate 0.5 on dyadic inputs (the scale is exactly 2: exact class), rate 0.1 on normal inputs; the first
    row's global index 0 and 8; with and without the residual, which joins after the mask; a dropped element is exactly the residual"""
    for N in G.G256_N:
        for rate, cls in ((0.5, 'dyadic'), (0.1, 'normal')):
            runs = [(form, True, False, (pa, pc, pr), (rate, row0)) for r, row0, form in G.G256_DROPS if r == rate for pa, pc, pr, _ in G.G256_PADS]
            _forward_case(dev, 'g256', M, K, N, cls, runs)


def test_both_kernels_meet_float64_at_one_shape(dev):
    """VF_SEL_GEMM_G256 = 0 sends a 256-tile shape to the 128-tile kernel: the same inputs, the same reference, the 128-tile kernel's
    constants.  Both kernels are held to float64, not to each other"""
    from viewformer_amd import _lib
    M, K, N = G.G256_BOTH
    runs = [('res', True, False, (8, 3, 5), None), ('bias', True, True, (8, 6, 0), None), ('gelu', True, True, (0, 0, 0), None),
            ('gelu_bwd', True, True, (8, 6, 5), None)]
    prev = _lib.select(_lib.SEL_GEMM_G256, 0)
    try:
        _forward_case(dev, 'direct', M, K, N, 'normal', runs)
        _forward_case(dev, 'direct', M, K, N, 'dyadic', runs[:2])
    finally:
        _lib.select(_lib.SEL_GEMM_G256, prev)
    _forward_case(dev, 'g256', M, K, N, 'normal', [(f, a, o, (8, 6, p[2]), d) for f, a, o, p, d in runs])
    _forward_case(dev, 'direct', M, K, N, 'normal', [('gelu_res', True, False, (8, 3, 5), None)])      # the form the 128-tile kernel keeps


# ------------------------------------------------------------------ tail tiles
@pytest.mark.parametrize('M,policy', G.TAIL_CASES)
def test_tail_tiles(dev, M, policy):
    """VF_SEL_GEMM_TAIL = 1 at K = 128, N = 4096: the policy restated (G.tail_policy) gives the tuple derived by hand; the first 256 rows,
    the 256 rows before the first tail tile and every tail row against float64; no sentinel left anywhere in the output"""
    from viewformer_amd import _lib
    K, N = G.TAIL_K, G.TAIL_N
    assert G.tail_policy(M, N) == policy
    inp = G.forward_inputs(M, K, N, 'normal', saved=False)
    wp = _pack(inp['W'], dev)
    rows = G.tail_rows(M, policy)
    pre0, mag0 = G.gemm(inp['x'][rows], inp['W'])
    prev = _lib.select(_lib.SEL_GEMM_TAIL, 1)
    try:
        for form, o16 in G.TAIL_FORMS:
            bufs = _launch(dev, inp, wp, form, True, o16, drop=G.TAIL_DROP, keep=True)
            got = {}
            for name, buf in bufs.items():
                if buf is not None:
                    assert not bool(torch.isnan(buf).any()) and not bool((buf == G.SENTINEL).any()), f'tail {form} {name}: an element was not written'
                    got[name] = buf[rows.to(dev)].cpu()
            _judge('tail', form, got, G.wants(form, inp, pre0, mag0, rows, G.TAIL_DROP), False, f'({M},{K},{N}) {form} o16 {o16}')
    finally:
        _lib.select(_lib.SEL_GEMM_TAIL, prev)


# ------------------------------------------------------------------ the weight gradient
def _tn_call(dev, x16, dy, M, K, N, splits, bias, record, pad):
    """vf_gemm_tn_bf16 through the C ABI -> (status, dW slabs [S][K][N] on the CPU, db slabs [S][N] or None).  ``record``: one array of
    records (weight slab | bias slab | four floats of padding) with slab_stride; else the two arrays with slab_stride 0"""
    xd, dd = _operand(x16, pad, dev), _operand(dy, pad, dev)
    rec = K * N + (N if bias else 0)
    if record:
        ws = torch.full((splits, rec + 4), G.SENTINEL, device=dev)
        bp = ctypes.c_void_p(ws.data_ptr() + K * N * 4) if bias else None
        stride = rec + 4
    else:
        ws = torch.full((splits, K * N), G.SENTINEL, device=dev)
        bs = torch.full((splits, N), G.SENTINEL, device=dev) if bias else None
        bp, stride = _P(bs), 0
    rc = _lib_().vf_gemm_tn_bf16(_P(xd), K + pad, _P(dd), 1 if dy.dtype == BF16 else 0, N + pad, M, K, N, splits, _P(ws), bp, stride, _strm())
    assert rc == 0, rc
    if record:
        what = f'tn record ({M},{K},{N}) splits {splits}'
        full = _result(ws, rec, what)
        return full[:, :K * N].reshape(splits, K, N), full[:, K * N:] if bias else None
    dW = _result(ws, K * N, 'tn w_slabs').reshape(splits, K, N)
    return dW, _result(bs, N, 'tn b_slabs') if bias else None


@pytest.mark.parametrize('M,K,N,splits', G.TN_CASES)
def test_weight_gradient_slab_by_slab(dev, M, K, N, splits):
    """every split's slab of dW and db on its own: grids of 1, 3, 5 and 6 workgroups, one chunk per split and uneven chunk ranges; dy
    float32 (db from the unrounded values) and bf16; with and without the bias slabs; the two slab layouts; ldx = K + 8, ldy = N + 8 with
    NaN in the padding"""
    for cls in ('dyadic', 'normal'):
        x16, dy = G.tn_inputs(M, K, N, cls)
        for y16 in (False, True):
            dyv = dy.to(BF16) if y16 else dy
            dW, mW, db, mb = G.gemm_tn(x16, dyv, splits)
            for y, bias, record, pad in G.TN_VARIANTS:
                if y != y16:
                    continue
                gW, gb = _tn_call(dev, x16, dyv, M, K, N, splits, bias, record, G.TN_PAD if pad else 0)
                what = f'({M},{K},{N}) splits {splits} {cls} dy16 {y16} bias {bias} record {record} pad {pad}'
                if cls == 'dyadic':
                    _exact('tn exact', gW, dW, what + ' dW')
                    if bias:
                        _exact('tn exact', gb, db, what + ' db')
                else:
                    _close('tn dW', gW, dW, mW, what)
                    if bias:
                        _close('tn db', gb, db, mb, what)


@pytest.mark.parametrize('splits', [1, 4])
def test_weight_gradient_selects(dev, splits):
    """x [256][256] with one 1 per row at column pi(m): dW[pi(m)] = bf16_rne(dy[m]) exactly, in the slab of m's split and 0 in the others"""
    M = K = N = 256
    xs, pi = G.selector(M, 620 + splits)
    _, dy = G.tn_inputs(M, K, N, 'normal')
    for dyv in (dy, dy.to(BF16)):
        want = G.gemm_tn(xs.to(BF16), dyv, splits)[0]
        assert R.mismatches(want.sum(0)[pi], G.bf16_rne(dyv.float())) == 0
        gW, _ = _tn_call(dev, xs.to(BF16), dyv, M, K, N, splits, False, False, G.TN_PAD)
        _exact('tn exact', gW, want, f'selector splits {splits} dy {dyv.dtype}')


@pytest.mark.parametrize('M,K,N,splits', G.TN_CASES)
def test_weight_gradient_folded(dev, M, K, N, splits):
    """ops.gemm_tn_bf16 (its own split count, contiguous operands) with accumulate on and off, db beside dw and right behind it (the single
    fold over K N + N floats): the folded sums against float64"""
    from viewformer_amd import ops
    for cls in ('dyadic', 'normal'):
        x16, dy = G.tn_inputs(M, K, N, cls)
        dw0, db0 = (G.eighths((K, N), 630), G.eighths((N,), 631)) if cls == 'dyadic' else (R.normal((K, N), 630), R.normal((N,), 631))
        for dyv in (dy, dy.to(BF16)):
            dW, mW, db, mb = G.gemm_tn(x16, dyv, 1)
            for acc in (False, True):
                wW, wmW = G.fold(dW, mW, dw0 if acc else None)
                wb, wmb = G.fold(db, mb, db0 if acc else None)
                for behind in (False, True):
                    flat = torch.cat((dw0.reshape(-1), db0)).to(dev)
                    dw = flat[:K * N].view(K, N)
                    dbt = flat[K * N:] if behind else db0.to(dev).clone()
                    ops.gemm_tn_bf16(x16.to(dev), dyv.to(dev), M, K, N, dw, dbt, accumulate=acc)
                    what = f'({M},{K},{N}) {cls} dy {dyv.dtype} accumulate {acc} behind {behind}'
                    if cls == 'dyadic':
                        _exact('tn exact', dw.cpu(), wW, what + ' dW')
                        _exact('tn exact', dbt.cpu(), wb, what + ' db')
                    else:
                        _close('tn dW', dw.cpu(), wW, wmW, what + ' folded')
                        _close('tn db', dbt.cpu(), wb, wmb, what + ' folded')


# ------------------------------------------------------------------ the slab fold
@pytest.mark.parametrize('nslabs', G.SLAB_COUNTS)
def test_sum_slabs(dev, nslabs):
    """((dst or 0) + slab 0) + slab 1 + ... in float32, bit for bit: 1 slab, the first batch of eight loads not full, full, one and nine
    slabs past it; one float4, 257 and one past the capped grid (compared on the device with the same float32 statement); a slab stride
    larger than n with NaN behind every slab; accumulate on and off"""
    lib = _lib_()
    for n in G.SLAB_N:
        for pad in (0, 8):
            gen = torch.Generator(device=dev).manual_seed(640 + nslabs)
            slabs = torch.full((nslabs, n + pad), float('nan'), device=dev)
            slabs[:, :n] = torch.randn((nslabs, n), generator=gen, device=dev) * torch.logspace(0, 2, nslabs, device=dev).view(-1, 1)
            dst0 = torch.randn((n,), generator=gen, device=dev)
            for acc in (False, True):
                dst = torch.full((n + 4,), G.SENTINEL, device=dev)
                dst[:n] = dst0
                assert lib.vf_sum_slabs_f32(_P(slabs), nslabs, n + pad, n, _P(dst), 1 if acc else 0, _strm()) == 0
                want = G.fold_f32([slabs[s, :n] for s in range(nslabs)], dst0 if acc else None)
                what = f'nslabs {nslabs} n {n} stride {n + pad} accumulate {acc}'
                assert bool((dst[n:] == G.SENTINEL).all()), f'sum_slabs {what}: wrote past n'
                _same_bits('sum_slabs', dst[:n] + 0.0, want + 0.0, what)                 # (+ 0.0: -0 and +0 are one value)
                if n <= 1028:
                    _exact('sum_slabs', dst[:n].cpu(), G.fold_f32([slabs[s, :n].cpu() for s in range(nslabs)], dst0.cpu() if acc else None), what + ' (CPU)')


# ------------------------------------------------------------------ the packings
@pytest.mark.parametrize('K,N', G.PACK_CASES)
def test_packings_agree_and_select(dev, K, N):
    """pack_dense_kn_bf16 of W [K][N], pack_dense_nk_bf16 of the first N rows of a [N + 2][K] transpose and pack_bf16_multi of both
    sources — the transposed one also at a base 4 bytes past a 16-byte boundary (the scalar path) — hold the same bits, and the selector
    GEMM through each returns bf16_rne(W)"""
    from viewformer_amd import ops
    lib = _lib_()
    W = R.normal((K, N), 660 + K + N, 0.05)
    Wd = W.to(dev)
    Wt = torch.cat((W.t(), R.normal((2, K), 661))).contiguous().to(dev)                    # [N + 2][K]
    n = int(lib.vf_gemm_bf16_packed_elems(K, N))
    packs = {'kn': ops.pack_dense_kn_bf16(Wd), 'nk': ops.pack_dense_nk_bf16(Wt, n_rows=N)}
    assert packs['kn'].numel() == n == -(-K // 64) * -(-N // 128) * 64 * 128
    off = torch.zeros(N * K + 4, device=dev)
    off[1:1 + N * K] = Wt[:N].reshape(-1)
    Wt_off = off[1:1 + N * K].view(N, K)
    assert Wt_off.data_ptr() % 16 == 4 and Wt_off.is_contiguous()
    outs = {k: torch.full((n + 8,), G.SENTINEL, dtype=BF16, device=dev) for k in ('multi kn', 'multi nk', 'multi nk off')}
    ops.pack_bf16_multi([(Wd, False, outs['multi kn']), (Wt[:N], True, outs['multi nk']), (Wt_off, True, outs['multi nk off'])])
    for k, o in outs.items():
        assert bool((o[n:] == G.SENTINEL).all()), f'{k}: wrote past the packing'
        packs[k] = o[:n]
    for k, p in packs.items():
        _same_bits('packings', p, packs['kn'], f'({K},{N}) {k}')
    x, pi = G.selector(K, 662 + K)
    inp = dict(x=x, W=W)
    for k, p in packs.items():
        _exact('packings', _launch(dev, inp, p.contiguous(), 'none', False, False)['out'], G.bf16_rne(W)[pi], f'({K},{N}) selector through {k}')


# ------------------------------------------------------------------ refusals: decided on the host, before any launch
def _refused(code, fn):
    from viewformer_amd import _lib
    with pytest.raises(_lib.VfError) as e:
        fn()
    assert f'({code})' in str(e.value), (code, str(e.value))


def test_forward_refusals(dev):
    """vf_gemm_bf16's own codes, as its launcher decides them in order (csrc/gemm_bf16.hip, vf_gemm_bf16_g256_launch): -1 bad argument,
    -2 unsupported.  The outputs keep their sentinel"""
    from viewformer_amd import ops
    B, Un = G.BAD_ARG, G.UNSUPPORTED
    M, K, N = 256, 128, 256
    W = R.normal((384, N), 670, 0.05).to(dev)
    wp = ops.pack_dense_kn_bf16(W)
    x32 = torch.zeros((M, 392), device=dev)
    x16 = x32.to(BF16)
    o32, o16 = _outbuf(M, N, 0, F32, dev), _outbuf(M, N, 0, BF16, dev)
    aux, res = _outbuf(M, N, 0, BF16, dev), torch.zeros((M, N), device=dev)
    kw = dict(bf16=True)
    _refused(Un, lambda: ops.igemm(x32, wp, M, 96, N, o32, lda=96, **kw))                                        # K % 64
    _refused(B, lambda: ops.igemm(x32, wp, M, K, N, o32, lda=K - 4, **kw))                                      # lda < K
    _refused(B, lambda: ops.igemm(x32, wp, M, K, N, o32, lda=K + 2, **kw))                                      # lda & 3
    _refused(B, lambda: ops.igemm(x16, wp, M, K, N, o32, lda=K + 4, a16=True, **kw))                            # bf16 x: lda & 7
    _refused(B, lambda: ops.igemm(x16, wp, M, K, N, o16, res=res, a16=True, o16=True, **kw))                    # bf16 out with a residual
    _refused(B, lambda: ops.igemm(x32, wp, 128, K, 128, o16, res=res, o16=True, **kw))                          # ... on the direct kernel's shapes
    _refused(Un, lambda: ops.igemm(x16, wp, M, K, N, o32, res=res, epilogue=ops.EPI_GELU_BWD, a16=True, **kw))  # GELU_BWD with float32 out
    _refused(B, lambda: ops.igemm(x16, wp, M, K, N, o32, epilogue=ops.EPI_GELU_DUAL, a16=True, **kw))           # DUAL without out_aux
    _refused(B, lambda: ops.igemm(x16, wp, M, K, N, o32, out_aux=aux, a16=True, **kw))                          # out_aux without DUAL
    for m, n in ((255, N), (M, 128)):                                                                           # DUAL and drop off the 256-tile shapes
        _refused(Un, lambda: ops.igemm(x16, wp, m, K, n, o32[:m, :n].contiguous(), epilogue=ops.EPI_GELU_DUAL, out_aux=aux[:m, :n].contiguous(), a16=True, **kw))
        _refused(Un, lambda: ops.igemm(x16, wp, m, K, n, o32, ldc=N, drop=(0.1, 1, 2, 0), a16=True, **kw))
    _refused(Un, lambda: ops.igemm(x16, wp, M, K, N, o32, drop=(0.1, 1, 2, 2), a16=True, **kw))                  # row0 % 4
    _refused(Un, lambda: ops.igemm(x16, wp, M, 192, N, o32, lda=192, a16=True, **kw))                           # bf16 x with K = 192
    _refused(Un, lambda: ops.igemm(x32, wp, M, 192, N, o16, lda=192, o16=True, **kw))                           # bf16 out with K = 192
    torch.cuda.synchronize()
    for t in (o32, o16, aux):
        assert bool((t == G.SENTINEL).all())


def test_weight_gradient_and_fold_refusals(dev):
    """vf_gemm_tn_bf16's and vf_sum_slabs_f32's own codes (csrc/gemm_tn_bf16.hip, csrc/gemm_x6.hip); nothing is written"""
    lib = _lib_()
    B, Un = G.BAD_ARG, G.UNSUPPORTED
    M, K, N = 128, 256, 256
    x = torch.zeros((M + 1, K + 8), dtype=BF16, device=dev)
    y32, y16 = torch.zeros((M + 1, N + 8), device=dev), torch.zeros((M + 1, N + 8), dtype=BF16, device=dev)
    ws = torch.full((2 * (K * N + N) + 8,), G.SENTINEL, device=dev)

    def tn(M=M, K=K, N=N, splits=2, ldx=K, ldy=N, y=y32, xp=None, yp=None, wp=None, stride=0, bias=False):
        return lib.vf_gemm_tn_bf16(xp or _P(x), ldx, yp or _P(y), 1 if y.dtype == BF16 else 0, ldy, M, K, N, splits, wp or _P(ws),
                                   ctypes.c_void_p(ws.data_ptr() + K * N * 4) if bias else None, stride, _strm())
    assert tn(K=128, ldx=128) == Un and tn(N=128, ldy=128) == Un and tn(M=96) == Un
    assert tn(ldx=K + 4) == Un                                                             # ldx & 7
    assert tn(ldy=N + 2) == Un and tn(ldy=N + 4, y=y16) == Un                              # ldy & 3 (float32 dy), ldy & 7 (bf16 dy)
    assert tn(ldx=K - 8) == B and tn(ldy=N - 4) == B
    assert tn(splits=3) == Un and tn(splits=0) == B                                        # splits > M / 64
    assert tn(xp=ctypes.c_void_p(x.data_ptr() + 8)) == Un and tn(yp=ctypes.c_void_p(y32.data_ptr() + 4)) == Un
    assert tn(wp=ctypes.c_void_p(ws.data_ptr() + 8)) == Un                                 # an operand base off 16 bytes
    assert tn(stride=K * N - 4) == B and tn(stride=K * N, bias=True) == B and tn(stride=K * N + N + 2, bias=True) == B
    assert tn(stride=K * N + N, bias=True) == 0                                            # one record exactly: taken
    torch.cuda.synchronize()
    assert bool((ws[2 * (K * N + N):] == G.SENTINEL).all()) and not bool((ws[:2 * (K * N + N)] == G.SENTINEL).any())
    dst = torch.full((16,), G.SENTINEL, device=dev)
    sl = torch.zeros((64,), device=dev)
    assert lib.vf_sum_slabs_f32(_P(sl), 2, 8, 6, _P(dst), 0, _strm()) == B                 # n & 3
    assert lib.vf_sum_slabs_f32(_P(sl), 2, 10, 8, _P(dst), 0, _strm()) == B                # stride & 3
    assert lib.vf_sum_slabs_f32(_P(sl), 0, 8, 8, _P(dst), 0, _strm()) == B
    torch.cuda.synchronize()
    assert bool((dst == G.SENTINEL).all())
