"""GPU: the transformer's (MIGT) row kernels one by one against the float64 references of tests/transformer_kernels_ref.py (pinned on the
CPU by tests/test_transformer_kernels_ref_host.py): transpose, embedding sum, row arg-max, uint8 post-process, column sums, LayerNorm
forward and backward, GELU forward and backward, the row softmax and the view-masked softmax with its backward, softmax cross-entropy,
AdamWeightDecay per tensor and over the flat buffer, the tiny dense layer.

Exact class (copies, selections, sums of three dyadic numbers, integer results, bf16 copies of a float32 result): the result must equal
the reference as values, element for element (R.mismatches == 0).  Rounded class: |got - want| <= c x 2^-24 x magnitude per element
(R.worst_ratio), the magnitude being the reference expression with every summand replaced by its absolute value.  ``TABLE`` below holds
one (basis, c) per kernel: the basis is the worst error the float32 CPU restatement of the kernel shows against float64 on these very
inputs, as the host file measures and prints it, and c = 4 x basis rounded up to a power of two (the factor covers another valid
summation order, fused multiply-adds and the device's expf / erff) — never a figure taken from the kernel.  A lost term, a stale tail, a
mask off by a view or a wrong tie lands orders of magnitude above.  Every kernel's measured worst ratio goes to the parity report
(profiles/transformer_kernels_parity.txt).

Shapes are the smallest at which each property can fail: every template width of the two LayerNorm kernels and its successor, a row count
that leaves dead slots in a 16-row block, the float4 column-sum kernel's tail branch and the narrow kernel, more than 256 splits, one
element past the capped grid of every grid-stride loop (compared on the device with the same float64 torch statement run there)."""
import ctypes

import numpy as np
import pytest
import torch

import training_kernels_ref as R
import transformer_kernels_ref as X
from conftest import parity_report

pytestmark = pytest.mark.gpu

# kernel: (basis, c).  basis = worst error of the float32 CPU restatement against float64 in units of 2^-24 x magnitude, as
# test_transformer_kernels_ref_host.py measures and prints it; c = 4 x basis, rounded up to a power of two.  'gelu_bwd bf16' is in units
# of its own bound, 2^-9 |want| + 1.5e-7 |df| (X.gelu_bwd_bf16_bound).  adamw_flat_ is judged with adamw_'s constant: the same formula
# per element, calibrated over both input sets.
TABLE = {
    'colsum': (0.53, 4.0),
    'layernorm': (3.00, 16.0),
    'layernorm_bwd': (2.57, 16.0),
    'gelu': (1.77, 8.0),
    'gelu_bwd': (2.26, 16.0),
    'gelu_bwd bf16': (1.87, 8.0),
    'softmax_rows_': (5.43, 32.0),
    'softmax_mask_': (4.56, 32.0),
    'softmax_mask_bwd_': (2.85, 16.0),
    'softmax_ce': (59.84, 256.0),
    'adamw_': (2.01, 16.0),
    'dense_small_k': (4.52, 32.0),
}
BASIS = {k: b for k, (b, c) in TABLE.items()}
C = {k: c for k, (b, c) in TABLE.items()}

BAD_ARG, UNSUPPORTED = -1, -2
_worst = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        kc = 'adamw_' if k == 'adamw_flat_' else k
        parity_report(test='transformer_kernels', kernel=k, worst_ratio=_worst[k], c=C.get(kc, 0.0), basis=BASIS.get(kc, 0.0),
                      unit=('its bound 2^-9 |want| + 1.5e-7 |df|' if k == 'gelu_bwd bf16' else '2^-24 x magnitude') if kc in C else 'mismatching elements')


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


# ------------------------------------------------------------------ exact class
@pytest.mark.parametrize('rows,cols', X.TRANSPOSE_SHAPES)
def test_transpose(dev, rows, cols):
    """below, on and above the 32 x 32 tile both ways; batches; ld_src > cols (the pad is not read into the result) and ld_dst > rows (the
    tail of every output row keeps its sentinel); a bf16 source is widened exactly"""
    from viewformer_amd import train_ops as T
    for batch, (ps, pd), bf16 in X.TRANSPOSE_VARIANTS:
        src = X.transpose_input(rows, cols, batch, ps, bf16)
        want, _ = X.transpose(src, rows, cols)
        ld_src, ld_dst = cols + ps, rows + pd
        out = torch.full((batch, cols, ld_dst), -777.0, device=dev)
        got = T.transpose(src.to(dev), rows, cols, ld_src=ld_src, batch=batch, bs_src=rows * ld_src, out=out, ld_dst=ld_dst)
        what = f'({rows},{cols}) batch {batch} pads {ps},{pd} bf16 {bf16}'
        _exact('transpose', got[:, :, :rows].cpu(), want, what)
        assert bool((got[:, :, rows:] == -777.0).all()), f'transpose {what}: the tail of an output row was written'
        if not ps:
            _exact('transpose', T.transpose(src.to(dev), rows, cols, batch=batch, bs_src=rows * cols).cpu(), want, what + ' default out')
    t = torch.zeros(64, device=dev)
    assert _lib_().vf_transpose_f32(_P(t), _P(t), 4, 4, 3, 4, 1, 0, 0, _strm()) == BAD_ARG          # ld_src < cols
    assert _lib_().vf_transpose_f32(_P(t), _P(t), 4, 4, 4, 3, 1, 0, 0, _strm()) == BAD_ARG          # ld_dst < rows


@pytest.mark.parametrize('BS,L,d,V', X.EMBED_CASES)
def test_embed_sum(dev, BS, L, d, V):
    """(tok + pos) + pose on the dyadic grid; ids include 0 and V - 1; d = 2048 and one float4 per row"""
    from viewformer_amd import ops
    ids, wte, wpe, add = X.embed_inputs(BS, L, d, V)
    got = ops.embed_sum(ids.to(dev), wte.to(dev), wpe.to(dev), add.to(dev), BS, L, d, V)
    _exact('embed_sum', got.cpu(), X.embed_sum(ids, wte, wpe, add, BS, L, d)[0], f'({BS},{L},{d},{V})')


@pytest.mark.parametrize('n', X.ARGMAX_N)
def test_argmax_rows(dev, n):
    """the first maximum of a row: n around the wave width and past 1024; ld = n + 4 with +3e38 in the pad; ties in neighbouring lanes and in
    one lane; an all-equal and an all -inf row give 0; a row holding +inf.  (NaN inputs have no defined answer and are not given.)"""
    from viewformer_amd import ops
    for rows in (1, 5):
        for kind in X.ARGMAX_KINDS:
            x = X.argmax_input(rows, n, kind)
            got = ops.argmax_rows(x.to(dev), rows, n, ld=n + X.ARGMAX_PAD)
            assert got.dtype == torch.int64
            _exact('argmax_rows', got.cpu(), X.argmax_rows(x, n)[0], f'n {n} rows {rows} {kind}')
        x = X.argmax_input(rows, n, 'plain')[:, :n].contiguous()
        _exact('argmax_rows', ops.argmax_rows(x.to(dev), rows, n).cpu(), X.argmax_rows(x, n)[0], f'n {n} rows {rows} ld = n')
    t = torch.zeros(8, device=dev)
    assert _lib_().vf_argmax_rows_f32(_P(t), 1, 4, 3, _P(torch.zeros(1, dtype=torch.int64, device=dev)), _strm()) == BAD_ARG


@pytest.mark.parametrize('n', [1, 255 * 5 + 6, X.POSTPROCESS_BIG])
def test_postprocess_u8(dev, n):
    """the two float32 neighbours either side of each of the 255 thresholds, and -3, -1, -0.0, 0, 1, 7: equal to the oracle's uint8.  n = 1
    is the threshold of 128 alone; the largest size repeats the values past the capped grid (second lap, compared on the device)"""
    from oracle import vqgan_oracle as vq
    from viewformer_amd import ops
    v = X.postprocess_input()
    assert v.numel() == 255 * 5 + 6
    if n == 1:
        x = v[127 * 5 + 2:127 * 5 + 3].to(dev)
    else:
        x = v.to(dev)[torch.arange(n, device=dev) % v.numel()]
    got = ops.postprocess_u8(x)
    assert got.dtype == torch.uint8
    _exact('postprocess_u8', got, vq.postprocess_u8(x.view(1, 1, 1, -1)).reshape(-1), f'n {n}')
    _exact('postprocess_u8', got, X.postprocess_u8(x)[0], f'n {n} (restatement)')


@pytest.mark.parametrize('d', X.LN_D)
def test_layernorm_bf16_copy(dev, d):
    """layernorm(out_bf16=True) is the round-to-nearest-even bf16 of layernorm's float32 rows, bit for bit"""
    from viewformer_amd import ops
    for rows in X.LN_ROWS:
        x, gamma, beta = (t.to(dev) for t in X.ln_inputs(rows, d))
        y = ops.layernorm(x, gamma, beta, rows, d, X.LN_EPS)
        y16 = ops.layernorm(x, gamma, beta, rows, d, X.LN_EPS, out_bf16=True)
        assert y16.dtype == torch.bfloat16
        _same_bits('layernorm bf16', y16, y.bfloat16(), f'rows {rows} d {d}')


@pytest.mark.parametrize('rows,d', X.LN_BWD_CASES)
def test_layernorm_bwd_bf16_copy_and_row_forms(dev, rows, d):
    """also_bf16 without dropout: the bf16 tensor is the bf16 rounding of the float32 dx of the same call; and the one-row and the two-row
    form of the kernel (VF_SEL_LN_BWD_TWO_ROWS = 0 / 1) give the same bits of dx, dgamma and dbeta on every case"""
    from viewformer_amd import _lib
    from viewformer_amd import train_ops as T
    dy, x, gamma, res, dg0, db0 = (t.to(dev) for t in X.ln_bwd_inputs(rows, d))
    prev = _lib.select(_lib.SEL_LN_BWD_TWO_ROWS, 1)
    try:
        for acc, with_res in X.LN_BWD_VARIANTS:
            out = {}
            for two in (1, 0):
                _lib.select(_lib.SEL_LN_BWD_TWO_ROWS, two)
                dg, db = dg0.clone(), db0.clone()
                dx, dx16 = T.layernorm_bwd(dy, x, gamma, dg, db, rows, d, X.LN_EPS, accumulate=acc, res=res if with_res else None, also_bf16=True)
                _same_bits('layernorm_bwd bf16', dx16, dx.bfloat16(), f'({rows},{d}) two_rows {two} accumulate {acc} res {with_res}')
                out[two] = (dx, dg, db)
            for nm, a, b in zip(('dx', 'dgamma', 'dbeta'), out[1], out[0]):
                _same_bits('layernorm_bwd row forms', a, b, f'({rows},{d}) accumulate {acc} res {with_res} {nm}')
    finally:
        _lib.select(_lib.SEL_LN_BWD_TWO_ROWS, prev)


@pytest.mark.parametrize('n', X.GELU_SIZES)
def test_gelu_bf16_copy(dev, n):
    """gelu(out_bf16=True) is the bf16 rounding of gelu's float32 result, bit for bit (both evaluate vf_gelu_erf)"""
    from viewformer_amd import train_ops as T
    u, _ = X.gelu_inputs(n, dev)
    f16 = T.gelu(u, out_bf16=True)
    assert f16.dtype == torch.bfloat16
    _same_bits('gelu bf16', f16, T.gelu(u).bfloat16(), f'n {n}')


# ------------------------------------------------------------------ rounded class
@pytest.mark.parametrize('M,N,ld', X.COLSUM_CASES)
def test_colsum(dev, M, N, ld):
    """(128,66,68) and (1000,260,260): the float4 kernel's tail branch; (1000,130,130) and (1,1,1): the one-column-per-thread kernel;
    32773 rows: more than 256 splits of 128 rows; the columns from N on hold 1e30; accumulate on a non-zero start and off"""
    from viewformer_amd import train_ops as T
    x, out0 = X.colsum_inputs(M, N, ld)
    xd = x.to(dev)
    for acc in (False, True):
        want, mag = X.colsum(x, out0, M, N, acc)
        out = torch.full((N + 4,), -777.0, device=dev)
        out[:N] = out0.to(dev)
        T.colsum(xd, out, M, N, ld=ld, accumulate=acc)
        _close('colsum', out[:N].cpu(), want, mag, f'({M},{N},{ld}) accumulate {acc}')
        assert bool((out[N:] == -777.0).all()), 'colsum wrote past N'
    ws = torch.empty(int(_lib_().vf_colsum_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    assert _lib_().vf_colsum_f32(_P(xd), _P(out), M, N, N - 1, 0, _P(ws), _strm()) == BAD_ARG


@pytest.mark.parametrize('d', X.LN_D)
def test_layernorm(dev, d):
    """every template width (256 / 512 / 1024 / 2048 features) at its upper edge and one float4 past it; one row and five (a block holds
    four); a constant row and a row of mean 100, std 0.01"""
    from viewformer_amd import ops
    eps = X.f32(X.LN_EPS)
    for rows in X.LN_ROWS:
        x, gamma, beta = X.ln_inputs(rows, d)
        want, mag = X.layernorm(x, gamma, beta, eps)
        got = ops.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), rows, d, X.LN_EPS)
        _close('layernorm', got.cpu(), want, mag, f'rows {rows} d {d}')


def test_layernorm_refuses_what_it_cannot_run(dev):
    t = torch.zeros(4 * 2052, device=dev)
    lib = _lib_()
    for fn in (lib.vf_layernorm_f32, lib.vf_layernorm_bf16out_f32):
        assert fn(_P(t), _P(t), _P(t), _P(t), 1, 2052, 1e-5, _strm()) == UNSUPPORTED
        assert fn(_P(t), _P(t), _P(t), _P(t), 1, 6, 1e-5, _strm()) == UNSUPPORTED
    ws = torch.zeros(int(lib.vf_layernorm_bwd_workspace_bytes(1, 1028)), dtype=torch.uint8, device=dev)
    for d in (1028, 6):
        assert lib.vf_layernorm_bwd_f32(_P(t), _P(t), _P(t), _P(t), _P(t), _P(t), 1, d, 1e-5, 0, None, None, 0.0, 0, 0, 0, _P(ws), _strm()) == UNSUPPORTED
    assert bool((t == 0).all())


@pytest.mark.parametrize('rows,d', X.LN_BWD_CASES)
def test_layernorm_bwd(dev, rows, d):
    """every template width (256 / 512 / 768 / 1024) at its edge and one float4 past it with 37 rows (two full 16-row blocks and five rows: a
    wave with a dead slot); 1, 3, 16, 17, 33 rows at d = 260; dgamma / dbeta accumulated onto a non-zero start and assigned; with and
    without the residual gradient"""
    from viewformer_amd import train_ops as T
    eps = X.f32(X.LN_EPS)
    dy, x, gamma, res, dg0, db0 = X.ln_bwd_inputs(rows, d)
    dyd, xd, gd, rd = dy.to(dev), x.to(dev), gamma.to(dev), res.to(dev)
    for acc, with_res in X.LN_BWD_VARIANTS:
        want, mag = X.layernorm_bwd(dy, x, gamma, eps, res if with_res else None, dg0 if acc else None, db0 if acc else None)
        dg, db = dg0.to(dev).clone(), db0.to(dev).clone()
        dx = T.layernorm_bwd(dyd, xd, gd, dg, db, rows, d, X.LN_EPS, accumulate=acc, res=rd if with_res else None)
        for nm, g, w_, m in zip(('dx', 'dgamma', 'dbeta'), (dx, dg, db), want, mag):
            _close('layernorm_bwd', g.cpu(), w_, m, f'({rows},{d}) accumulate {acc} res {with_res} {nm}')


@pytest.mark.parametrize('n', X.GELU_SIZES)
def test_gelu_and_its_backward(dev, n):
    """u sweeps [-12, 12] in steps of 2^-6 with 0, -0.0 and +/-1e-30; n = 32768 x 256 + 5 is the loop's second lap"""
    from viewformer_amd import train_ops as T
    big = n > 1 << 20
    u, df = X.gelu_inputs(n, dev if big else 'cpu')
    ud, dfd = u.to(dev), df.to(dev)
    want, mag = X.gelu(u)
    _close('gelu', T.gelu(ud) if big else T.gelu(ud).cpu(), want, mag, f'n {n}')
    want, mag = X.gelu_bwd(u, df)
    got = T.gelu_bwd(ud, dfd)
    _close('gelu_bwd', got if big else got.cpu(), want, mag, f'n {n}')
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize('n', X.GELU_SIZES)
def test_gelu_bwd_bf16(dev, n):
    """the bf16-output backward (erf by Abramowitz & Stegun 7.1.26) against 2^-9 |want| + 1.5e-7 |df| per element"""
    from viewformer_amd import train_ops as T
    big = n > 1 << 20
    u, df = X.gelu_inputs(n, dev if big else 'cpu')
    want, _ = X.gelu_bwd(u, df)
    got = T.gelu_bwd(u.to(dev), df.to(dev), out_bf16=True)
    assert got.dtype == torch.bfloat16
    _close('gelu_bwd bf16', got.float() if big else got.float().cpu(), want, X.gelu_bwd_bf16_bound(want, df), f'n {n}')


@pytest.mark.parametrize('rows', [1, 5, 1027])
def test_softmax_rows(dev, rows):
    """row lengths around the wave width and 1000; one row nearly one-hot; scale 1 and 2^-4"""
    from viewformer_amd import ops
    for r, n in X.SOFTMAX_CASES:
        if r != rows:
            continue
        x = X.softmax_logits(rows, n)
        for scale in (1.0, 0.0625):
            want, mag = X.softmax_rows(x, scale)
            got = ops.softmax_rows_(x.to(dev).clone(), rows, n, scale)
            _close('softmax_rows_', got.cpu(), want, mag, f'rows {rows} n {n} scale {scale}')


@pytest.mark.parametrize('case', X.MASK_CASES)
def test_softmax_mask_and_its_backward(dev, case):
    """the three mask specs (streams, twin views, plain with a last view of 4 tokens), no mask, one token, one view that is not full; a
    masked probability and a masked ds are exactly 0 (magnitude 0); the backward takes the float32 rounding of the reference's p"""
    from viewformer_amd import train_ops as T
    batch, Tn, L, spec, scale = case
    s, dp = X.mask_inputs(batch, Tn, L, spec)
    want, mag = X.softmax_mask(s, Tn, L, spec, scale)
    got = T.softmax_mask_(s.to(dev).clone(), batch, Tn, L, spec, scale)
    _close('softmax_mask_', got.cpu(), want, mag, str(case))
    p = want.float()
    want, mag = X.softmax_mask_bwd(p, dp, Tn, L, spec, scale)
    _close('softmax_mask_bwd_', T.softmax_mask_bwd_(p.to(dev), dp.to(dev).clone(), batch, Tn, L, spec, scale).cpu(), want, mag, str(case))


def _ce_check(dev, rows, V, spread):
    from viewformer_amd import train_ops as T
    logits, t, w = X.ce_inputs(rows, V, spread)
    for e in X.CE_SMOOTHING:
        (wl, wd), (ml, md) = X.softmax_ce(logits, t, w, X.f32(e))
        loss, dl = T.softmax_ce(logits.to(dev), t.to(dev), w.to(dev), rows, V, e)
        what = f'rows {rows} V {V} smoothing {e}' + (' spread' if spread else '')
        _close('softmax_ce', loss.cpu(), wl, ml, what + ' loss')
        _close('softmax_ce', dl.cpu(), wd, md, what + ' dlogits')


@pytest.mark.parametrize('rows', X.CE_ROWS)
def test_softmax_ce(dev, rows):
    """V around the wave width, 1 and 1026; label smoothing 0 and 0.1; weights with exact zeros (their rows' gradient is exactly 0);
    targets 0 and V - 1 planted, all inside [0, V)"""
    for V in X.CE_V:
        _ce_check(dev, rows, V, False)


def test_softmax_ce_with_logits_spread_over_120(dev):
    _ce_check(dev, *X.CE_SPREAD, True)


@pytest.mark.parametrize('n', X.ADAMW_SIZES)
def test_adamw(dev, n):
    """elements with g = 0, m = 0, v = 0 planted; the reference forms 1 - beta from the float32 betas, as the kernel does;
    n = 8192 x 256 + 3 is the loop's second lap"""
    from viewformer_amd import train_ops as T
    big = n > 1 << 20
    hyper = X.adamw_hyper()
    p, g, m, v = X.adamw_inputs(n, dev if big else 'cpu')
    want, mag = X.adamw(p, g, m, v, *hyper)
    pd, gd, md, vd = (t.to(dev).clone() for t in (p, g, m, v))
    T.adamw_(pd, gd, md, vd, *hyper)
    for nm, got, w_, m_ in zip(('param', 'm', 'v'), (pd, md, vd), want, mag):
        _close('adamw_', got if big else got.cpu(), w_, m_, f'n {n} {nm}')
    assert torch.equal(gd, g.to(dev))


@pytest.mark.parametrize('name', list(X.ADAMW_FLAT_RANGES))
def test_adamw_flat(dev, name):
    """no range, one at offset 0, two adjacent ranges, a last range ending at n, 256 ranges (the whole LDS table): bit-identical to adamw_
    run tensor by tensor (lr_decay = 0 inside a range), and against the float64 reference with the ranges as a mask"""
    from viewformer_amd import train_ops as T
    n, ranges = X.ADAMW_FLAT_N, X.ADAMW_FLAT_RANGES[name]
    ld, la, b1, b2, eps = X.adamw_hyper()
    p, g, m, v = X.adamw_inputs(n)
    want, mag = X.adamw(p, g, m, v, ld, la, b1, b2, eps, nodecay=X.nodecay_mask(n, ranges))
    pf, gf, mf, vf = (t.to(dev).clone() for t in (p, g, m, v))
    rt = torch.tensor(ranges, dtype=torch.int64, device=dev).view(-1, 2) if ranges else None
    T.adamw_flat_(pf, gf, mf, vf, rt, ld, la, b1, b2, eps)
    pt, mt, vt = (t.to(dev).clone() for t in (p, m, v))
    for a, b, nodecay in X.segments(n, ranges):
        T.adamw_(pt[a:b], gf[a:b], mt[a:b], vt[a:b], 0.0 if nodecay else ld, la, b1, b2, eps)
    for nm, flat, per, w_, m_ in zip(('param', 'm', 'v'), (pf, mf, vf), (pt, mt, vt), want, mag):
        _same_bits('adamw_flat_ = adamw_', flat, per, f'{name} {nm}')
        _close('adamw_flat_', flat.cpu(), w_, m_, f'{name} {nm}', c=C['adamw_'])


def test_adamw_flat_refuses_what_it_cannot_run(dev):
    lib = _lib_()
    n = 64
    buf = [torch.ones(n + 8, device=dev) for _ in range(4)]
    many = torch.tensor([(4 * k, 4 * k + 4) for k in range(257)], dtype=torch.int64, device=dev)
    hyper = X.adamw_hyper()

    def call(ts, count, rt, nr):
        return lib.vf_adamw_flat_f32(_P(ts[0]), _P(ts[1]), _P(ts[2]), _P(ts[3]), count, _P(rt), nr, *hyper, _strm())
    assert call(buf, n, many, 257) == UNSUPPORTED                                         # one more range than the table holds
    assert call(buf, n - 2, None, 0) == UNSUPPORTED                                       # n no multiple of 4
    for k in range(4):                                                                    # each pointer in turn off its 16-byte boundary
        assert call([t[1:] if i == k else t for i, t in enumerate(buf)], n, None, 0) == UNSUPPORTED
    assert all(bool((t == 1.0).all()) for t in buf)
    assert call(buf, n, many, 256) == 0


@pytest.mark.parametrize('rows,K,N', X.DENSE_K_CASES)
def test_dense_small_k(dev, rows, K, N):
    """K = 1, 7, 16; N = 129 leaves a ragged last block; GELU on and off; with and without the bias; K = 17 is refused"""
    from viewformer_amd import ops
    x, W, b = X.dense_k_inputs(rows, K, N)
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
    for gelu_on in (False, True):
        for bias, biasd in ((b, bd), (None, None)):
            want, mag = X.dense_small_k(x, W, bias, gelu_on)
            _close('dense_small_k', ops.dense_small_k(xd, Wd, biasd, rows, K, N, gelu_on).cpu(), want, mag,
                   f'({rows},{K},{N}) gelu {gelu_on} bias {bias is not None}')
    assert _lib_().vf_dense_small_k_gelu_f32(_P(xd), _P(Wd), _P(bd), _P(torch.empty(N, device=dev)), 1, 17, 1, 0, _strm()) == UNSUPPORTED
