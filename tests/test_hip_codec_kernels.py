"""GPU: the image codec's glue kernels one by one against the float64 references of tests/codec_kernels_ref.py (pinned on the CPU by
tests/test_codec_kernels_ref_host.py), at the shapes the 128-px model never asks for: the generic GroupNorm prologue of the 1x1 GEMMs
and row tiles that straddle images, the statistics at every lane count / split tail / group count, the finalize around its 512-slot
fork, the apply's second grid lap, strided and peaked spatial attention, the codebook kernels on their own, conv_in at odd sizes and
on its second lap, and the convolution to a handful of channels up to its LDS limit.

Rules.  Native f32 kernels: c x 2^-24 x magnitude per element with ``C`` below: 4 x the worst error of the float32 CPU restatement of
the kernel's summation order on these very inputs (the host file's calibration), rounded up to a power of two, never a figure of the
kernel.  Behind a swish the swish's own figure is added (vf_common.h: vf_swish 4, vf_swish_1ulp 3 units of 2^-24 x |value|).  x6 / x3h
arms: the standing claim (max error < 6e-7 of magnitude, rms < 1.25 x the native f32 arm's + 1e-9; conv_in: 4e-7; attention:
e3h < 1.25 e32 + 2e-7 max(1, |ref|)).  Statistics: the variance rule, per (image, group)
    |rstd error| / rstd <= 1/2 c_gn 2^-24 (mean^2 + var) / (var + eps) + 2^-23,      |mean error| <= c 2^-24 (|mean| + std):
the kernel adds fp32 sums and sums of squares, so the error of var scales with mean^2 + var, not with var.  Exact classes: 0 differing
elements.  Every refusal is a VfError with the entry point's own code.  Every worst figure goes to the parity report
(profiles/codec_kernels_parity.txt)."""
import time

import numpy as np
import pytest
import torch

import codec_kernels_ref as K
import conv_kernels_ref as CR
from conftest import parity_report

pytestmark = pytest.mark.gpu

# c = 4 x basis rounded up to a power of two; basis = worst error of the float32 CPU restatement against float64 in units of
# 2^-24 x magnitude, as test_codec_kernels_ref_host.py measures and prints it (recorded in profiles/codec_kernels_parity.txt)
C = {
    'gn_mean': 32.0,               # basis 5.27
    'gn_var': 64.0,                # basis 11.06  (c_gn of the variance rule)
    'apply': 16.0,                 # basis 2.63
    'gemm_pro': 8.0,               # basis 1.39
    'attn_s': 32.0,                # basis 5.20  (scores of the selector and random classes)
    'attn_s_shift': 256.0,         # basis 41.84 (scores of the shifted classes: 1280 or more enters the chain first, every later sum is rounded at its size)
    'attn_pv': 32.0,               # basis 6.21  (softmax and P V)
    'colsumsq': 64.0,              # basis 13.25
    'conv_in': 32.0,               # basis 5.33
    'small': 16.0,                 # basis 3.72
}
BAD_ARG, UNSUPPORTED = r'\(-1\)', r'\(-2\)'
GN_CODEC_TOL = 1e-5                # the tolerance test_hip_ops.py::test_groupnorm_stats has always claimed

_worst = {}


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.0), float(v))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        parity_report(test='codec_kernels', kernel=k, worst=_worst[k], c=C.get(k.split(':')[0], ''))


def _id(row):
    return '-'.join(str(v) for v in row)


def _refused(code, fn, *a, **kw):
    from viewformer_amd import _lib
    with pytest.raises(_lib.VfError, match=code):
        fn(*a, **kw)
        torch.cuda.synchronize()


class _Null:
    """a missing pointer where a wrapper asks its argument for data_ptr()"""
    def data_ptr(self):
        return None


# ================================================================== GroupNorm statistics
@pytest.mark.parametrize('cls', K.STATS_CLASSES, ids=str)
@pytest.mark.parametrize('row', K.STATS_ROWS, ids=_id)
def test_groupnorm_stats_meet_the_variance_rule(dev, row, cls):
    from viewformer_amd import ops
    Cc, groups, HW = row
    x, gamma = K.stats_inputs(row, cls)
    mean_c, scale_c = ops.groupnorm_stats(x.to(dev), gamma.to(dev), K.STATS_N, HW, Cc, groups, 1e-6)
    ok, wm, ws = K.stats_within(mean_c.cpu(), scale_c.cpu(), x, gamma, row, C['gn_mean'], C['gn_var'])
    _note('gn_mean:stats error / bound', wm)
    _note('gn_var:stats scale error / bound', ws)
    print(f'{row} {cls}: mean error {wm:.3f} of its bound (c = {C["gn_mean"]:g}), scale error {ws:.3f} of the variance rule (c_gn = {C["gn_var"]:g})')
    assert ok, (row, cls, wm, ws)
    assert float(scale_c[:, 0].abs().max()) == 0.0 and bool((scale_c[:, Cc - 1] < 0).all())        # gamma = 0 / gamma < 0


def test_groupnorm_stats_refusals(dev):
    from viewformer_amd import ops
    for Cc, groups in K.STATS_REFUSED:
        x, gamma = torch.zeros((3 * 8, Cc), device=dev), torch.ones(Cc, device=dev)
        _refused(UNSUPPORTED, ops.groupnorm_stats, x, gamma, 3, 8, Cc, groups)


@pytest.mark.parametrize('row', K.FIN_ROWS, ids=_id)
def test_groupnorm_finalize_against_float64_of_the_partials(dev, row):
    from viewformer_amd import ops
    n, ns, Cc, groups = row
    cg = Cc // groups
    part, gamma, HW = K.finalize_inputs(row)
    mean_c, scale_c = (t.cpu() for t in ops.groupnorm_finalize(part.to(dev), gamma.to(dev), n, HW, Cc, groups))
    mean, var, rstd = K.finalize_ref(part, HW, cg)
    bm, br = K.finalize_bounds(part, HW, cg, ns)
    rm, rs = K.gn_channels(mean, rstd, gamma, Cc)
    okm, wm = K.within(mean_c, rm, bm.repeat_interleave(cg, 1))
    oks, ws = K.within(scale_c, rs, (br * rstd).repeat_interleave(cg, 1) * K.t64(gamma).abs())
    _note('finalize mean error / bound', wm)
    _note('finalize scale error / bound', ws)
    print(f'{row}: {"eight-lane" if ns <= 512 else "wave"} kernel, mean error {wm:.3f}, scale error {ws:.3f} of their bounds')
    assert okm and oks, (row, wm, ws)
    # a slightly negative variance is clamped: rstd = 1 / sqrt(eps) exactly
    assert float(var[0, 0]) < 0
    assert torch.equal(scale_c[0, :cg], torch.tensor(np.float32(1.0 / np.sqrt(K.EPS))) * gamma[:cg])


@pytest.mark.parametrize('swish', [False, True], ids=['lin', 'swish'])
@pytest.mark.parametrize('row', K.APPLY_ROWS + [K.APPLY_LAP], ids=_id)
def test_groupnorm_apply(dev, row, swish):
    from viewformer_amd import ops
    Cc, HW, n = row
    x, mean_c, scale_c, beta = K.apply_inputs(row)
    got = ops.groupnorm_apply(x.to(dev), mean_c.to(dev), scale_c.to(dev), beta.to(dev), n, HW, Cc, swish).cpu()
    ref, mag = K.apply_ref(x, mean_c, scale_c, beta, n, HW, Cc, swish)
    ok, w = K.within(got, ref, K.apply_bound(C['apply'], ref, mag, swish))
    _note('apply:error / bound' + (' (swish)' if swish else ''), w)
    print(f'{row} swish={swish}: worst error {w:.3f} of its bound (c = {C["apply"]:g}' + (f', vf_swish {K.SWISH_U:g} units)' if swish else ')'))
    assert ok, (row, swish, w)


def test_groupnorm_apply_refuses_six_channels(dev):
    from viewformer_amd import ops
    z = torch.zeros((3 * 8, 6), device=dev)
    _refused(BAD_ARG, ops.groupnorm_apply, z, torch.zeros((3, 6), device=dev), torch.ones((3, 6), device=dev), torch.zeros(6, device=dev), 3, 8, 6, False)


# ================================================================== GroupNorm prologue of the 1x1 GEMM
def _pro_launch(arm, row, inp, swish, dev, pro=None, rpi=None):
    """one launch on rows of leading dimension C + 4 (NaN behind), out / res the leading columns of [M][N + 4] / [M][N + 8] buffers"""
    from viewformer_amd import ops
    x, mc, sc, beta, w, b, res = inp
    r, n, N, _ = row
    Cc, M = K.PRO_C, r * n
    xbuf = torch.full((M, Cc + 4), float('nan'), device=dev)
    xbuf[:, :Cc] = x.to(dev)
    obuf = torch.full((M + 1, N + 4), -777.0, device=dev)
    rbuf = None
    if res is not None:
        rbuf = torch.full((M, N + 8), 555.0, device=dev)
        rbuf[:, :N] = res.to(dev)
    wd = w.to(dev)
    wp = ops.pack_dense_kn(wd) if arm == 'f32' else ops.pack_dense_kn_x6(wd) if arm == 'x6' else ops.pack_dense_kn_x3h(wd)
    pro = (mc.to(dev), sc.to(dev), beta.to(dev)) if pro is None else pro
    ops.igemm(xbuf, wp, M, Cc, N, obuf, bias=None if b is None else b.to(dev), res=rbuf, pro=pro, pro_swish=swish,
              pro_rows_per_img=r if rpi is None else rpi, lda=Cc + 4, ldc=N + 4, ldr=N + 8, x6=arm == 'x6', x3h=arm == 'x3h')
    torch.cuda.synchronize()
    assert bool((obuf[:M, N:] == -777.0).all()) and bool((obuf[M:] == -777.0).all()), f'{arm} {row}: the sentinels behind the output were written'
    return obuf[:M, :N].cpu()


def _err(out, ref, mag):
    e = (out.double() - ref).abs() / mag
    return float(e.max()), float(e.pow(2).mean().sqrt())


@pytest.mark.parametrize('swish', [False, True], ids=['lin', 'swish'])
@pytest.mark.parametrize('row', K.PRO_ROWS, ids=_id)
def test_gemm_groupnorm_prologue(dev, row, swish):
    inp = K.pro_inputs(row)
    ref, mag, MAG = K.pro_ref(row, inp, swish)
    form = K.pro_form(row[0])
    o32 = _pro_launch('f32', row, inp, swish, dev)
    ok, w = K.within(o32, ref, K.pro_bound(C['gemm_pro'], mag, MAG, swish, K.SWISH_U))
    mx32, rms32 = _err(o32, ref, mag)
    _note('gemm_pro:f32 error / bound', w)
    print(f'{row} swish={swish}: f32 worst {w:.3f} of its bound (c = {C["gemm_pro"]:g}), max {mx32:.2e} rms {rms32:.2e} of magnitude')
    fails = [] if ok else [f'f32: {w:.3f} of its bound']
    for arm in ('x6', 'x3h'):
        mx, rms = _err(_pro_launch(arm, row, inp, swish, dev), ref, mag)
        _note(f'max:{arm} prologue {form}', mx)
        _note(f'rms/f32:{arm} prologue {form}', rms / (rms32 + 1e-30))
        print(f'{row} swish={swish}: {arm} ({form}) max {mx:.2e} rms {rms:.2e} | f32 rms {rms32:.2e}')
        if not (mx < K.X6_MAX and rms < K.X6_RMS * rms32 + 1e-9):
            fails.append(f'{arm}: max {mx:.2e} rms {rms:.2e} against f32 rms {rms32:.2e}')
    assert not fails, f'{row} swish={swish}: ' + '; '.join(fails)


def test_gemm_groupnorm_prologue_refusals(dev):
    row = K.PRO_ROWS[1]
    inp = K.pro_inputs(row)
    mc, sc, beta = (t.to(dev) for t in inp[1:4])
    for arm in K.PRO_ARMS:
        _refused(BAD_ARG, _pro_launch, arm, row, inp, False, dev, rpi=0)
        for pro in ((_Null(), sc, beta), (mc, _Null(), beta), (mc, sc, _Null())):
            _refused(BAD_ARG, _pro_launch, arm, row, inp, False, dev, pro=pro)


# ================================================================== spatial attention
def _attn_launch(q, k, v, x3h, dev, ld=None, ldo=None):
    from viewformer_amd import ops
    n, HW, Cc = q.shape
    ld, ldo = 3 * Cc + 8 if ld is None else ld, Cc + 4 if ldo is None else ldo
    qkv = torch.full((n * HW * ld + 64,), float('nan'), device=dev)
    qkv[:n * HW * ld] = K.attn_pack(q, k, v, ld).to(dev).view(-1)
    out = torch.full((n * HW * ldo + 64,), -777.0, device=dev)
    ov = out[:n * HW * ldo].view(n * HW, ldo)
    ops.attn_spatial(qkv[:n * HW * ld].view(n * HW, ld)[:, :3 * Cc], n, HW, Cc, K.attn_scale(Cc), out=ov[:, :Cc], x3h=x3h)
    torch.cuda.synchronize()
    assert bool((ov[:, Cc:] == -777.0).all()) and bool((out[n * HW * ldo:] == -777.0).all()), 'the sentinels in the gap / behind the output were written'
    return ov[:, :Cc].cpu().view(n, HW, Cc)


@pytest.mark.parametrize('cls', K.ATTN_CLASSES)
@pytest.mark.parametrize('n', K.ATTN_N)
@pytest.mark.parametrize('shape', K.ATTN_SHAPES, ids=_id)
def test_attn_spatial(dev, shape, n, cls):
    HW, Cc = shape
    q, k, v = K.attn_inputs(cls, HW, Cc, n)
    ref, M, S, _, _ = K.attn_ref(q, k, v, K.attn_scale(Cc))
    o32, o3h = _attn_launch(q, k, v, False, dev), _attn_launch(q, k, v, True, dev)
    fails = []
    if cls == 'exact':
        bad = K.mismatches(o32, ref)
        _note('exact:attn_spatial_f32', bad)
        if bad:
            fails.append(f'f32: {bad} of {ref.numel()} elements differ')
    else:
        c_s = C[K.attn_score_key(cls)]
        ok, w = K.within(o32, ref, K.attn_bound(C['attn_pv'], c_s, M, S))
        _note(f'attn_pv:f32 error / bound ({cls})', w)
        print(f'{shape} n={n} {cls}: f32 worst {w:.3f} of its bound (c_pv = {C["attn_pv"]:g}, c_s = {c_s:g}, largest score magnitude {float(S.max()):.1f})')
        if not ok:
            fails.append(f'f32: {w:.3f} of its bound')
    if cls == 'selector':                             # the output is row pi(i) of v, to fp32 rounding (+ the off-target mass)
        want = K.t64(v)[:, torch.from_numpy(K.attn_perm(HW))]
        ok, w = K.within(o32, want, K.U * want.abs() + 2.0 ** -40 * float(want.abs().max()))
        if not ok:
            fails.append(f'f32: selector {w:.2f} roundings from the selected row')
    e32, e3h = float((o32.double() - ref).abs().max()), float((o3h.double() - ref).abs().max())
    _note(f'x3h - 1.25 f32 ({cls})', e3h - K.ATTN_X3H_MUL * e32)
    print(f'{shape} n={n} {cls}: f32 err {e32:.2e}  x3h err {e3h:.2e}')
    if not e3h < K.ATTN_X3H_MUL * e32 + K.ATTN_X3H_ABS * max(1.0, float(ref.abs().max())):
        fails.append(f'x3h: {e3h:.2e} against f32 {e32:.2e}')
    assert not fails, f'{shape} n={n} {cls}: ' + '; '.join(fails)


def test_attn_spatial_refusals_and_the_empty_batch(dev):
    from viewformer_amd import ops
    q, k, v = K.attn_inputs('random', 128, 256, 1)
    for x3h in (False, True):
        _refused(UNSUPPORTED, _attn_launch, q, k, v, x3h, dev)
        HW, Cc = 64, 256
        buf = torch.zeros(HW * (3 * Cc + 8), device=dev)
        out = torch.full((HW * (Cc + 4),), -777.0, device=dev)
        o = out.view(HW, Cc + 4)[:, :Cc]
        view = lambda ld: buf.as_strided((HW, 3 * Cc), (ld, 1))                   # noqa: E731
        _refused(BAD_ARG, ops.attn_spatial, view(3 * Cc + 2), 1, HW, Cc, 0.0625, out=o, x3h=x3h)
        _refused(BAD_ARG, ops.attn_spatial, view(3 * Cc - 4), 1, HW, Cc, 0.0625, out=o, x3h=x3h)
        _refused(BAD_ARG, ops.attn_spatial, view(3 * Cc), 1, HW, Cc, 0.0625, out=out.as_strided((HW, Cc), (Cc - 4, 1)), x3h=x3h)
        ops.attn_spatial(view(3 * Cc + 8), 0, HW, Cc, 0.0625, out=o, x3h=x3h)        # n = 0: returns, out untouched
        torch.cuda.synchronize()
        assert bool((out == -777.0).all())


# ================================================================== codebook
@pytest.mark.parametrize('shape', K.CB_SHAPES, ids=_id)
def test_colsumsq_and_gather(dev, shape):
    from viewformer_amd import ops
    D, Kc = shape
    E = K.codebook(D, Kc)
    _, e_sq = ops.vq_pack_codebook(E.to(dev))
    ref = K.t64(E).pow(2).sum(0)
    r = K.worst_ratio(e_sq.cpu(), ref, ref)
    _note('colsumsq', r)
    print(f'{shape}: colsumsq worst {r:.2f} x 2^-24 x magnitude (c = {C["colsumsq"]:g})')
    assert r <= C['colsumsq']
    idx = K.gather_indices(Kc)
    got = ops.codebook_gather(E.to(dev), idx.to(dev), D, Kc).cpu()
    bad = K.mismatches(got, K.gather_ref(E, idx))
    _note('exact:codebook_gather', bad)
    assert bad == 0 and torch.equal(got[3], E[:, 0]) and torch.equal(got[11], E[:, Kc - 1])      # indices -5 and Kc + 3 are clamped
    # M = 0 is a no-op on both kernels (an empty tensor hands over a null pointer)
    assert tuple(ops.codebook_gather(E.to(dev), idx[:0].to(dev), D, Kc).shape) == (0, D)
    Ep, _ = ops.vq_pack_codebook(E.to(dev))
    assert ops.vq_argmin(torch.empty((0, D), device=dev), Ep, e_sq, D, Kc).numel() == 0


def _lookup(z, E, dev):
    from viewformer_amd import ops
    D, Kc = E.shape
    Ep, esq = ops.vq_pack_codebook(E.to(dev))
    return ops.vq_argmin(z.to(dev), Ep, esq, D, Kc).cpu()


@pytest.mark.parametrize('row', K.LOOKUP_ROWS, ids=_id)
def test_vq_argmin_planted_class(dev, row):
    z, E, k, _ = K.planted_inputs(row)
    idx = _lookup(z, E, dev)
    bad = int((idx != k).sum())
    _note('exact:vq_argmin planted', bad)
    assert bad == 0, f'{row}: {bad} of {row[0]} planted codes missed: rows {torch.nonzero(idx != k).view(-1)[:8].tolist()}'


@pytest.mark.parametrize('row', K.LOOKUP_ROWS, ids=_id)
def test_vq_argmin_random_class(dev, row):
    z, E = K.random_lookup_inputs(row)
    ok, share, msg = K.lookup_check(_lookup(z, E, dev), z, E)
    _note('vq_argmin random: exempt share', share)
    assert ok and share <= 0.01, (row, msg, share)


def test_vq_exact_ties_resolve_to_the_lowest_index_across_tiles_and_half_waves(dev):
    z, E, want = K.tie_inputs()
    assert _lookup(z, E, dev).tolist() == want


def test_vq_argmin_refuses_a_depth_of_48(dev):
    from viewformer_amd import ops
    z = torch.zeros((4, 48), device=dev)
    _refused(UNSUPPORTED, ops.vq_argmin, z, torch.zeros(64 * 128, device=dev), torch.zeros(64, device=dev), 48, 64)


# ================================================================== conv_in
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'no_bias'])
@pytest.mark.parametrize('row', K.CONV_IN_ROWS, ids=_id)
def test_conv_in_valu_form(dev, row, bias):
    from viewformer_amd import ops
    cout, n, H, W = row
    img, w, b = K.conv_in_inputs(row)
    b = b if bias else None
    bd = b.to(dev) if bias else None
    o8 = ops.conv_in(img.to(dev), w.to(dev), bd, n, H, W, cout).cpu()
    of = ops.conv_in(K.preprocess_u8(img).to(dev), w.to(dev), bd, n, H, W, cout).cpu()
    assert torch.equal(o8, of), 'the u8 and the f32 entry differ on the same pixel values'
    ref, mag = K.conv_in_ref(img, w, b)
    r = K.worst_ratio(o8, ref, mag)
    _note('conv_in', r)
    print(f'{row} bias={bias}: worst {r:.2f} x 2^-24 x magnitude (c = {C["conv_in"]:g})')
    assert r <= C['conv_in']


@pytest.mark.parametrize('row', K.CONV_IN_LAPS, ids=_id)
def test_conv_in_second_lap_equals_its_single_lap_launches(dev, row):
    from viewformer_amd import ops
    cout, n, H, W = row
    img, w, b = K.conv_in_inputs(row)
    imgd, wd, bd = img.to(dev), w.to(dev), b.to(dev)
    out = ops.conv_in(imgd, wd, bd, n, H, W, cout)
    for i in range(n):
        assert torch.equal(out[i], ops.conv_in(imgd[i:i + 1].contiguous(), wd, bd, 1, H, W, cout)[0]), f'image {i} differs from its own launch'
    for i in (0, n - 1):
        ref, mag = K.conv_in_ref(img[i:i + 1], w, b)
        r = K.worst_ratio(out[i:i + 1].cpu(), ref, mag)
        _note('conv_in', r)
        assert r <= C['conv_in'], (row, i, r)


def test_conv_in_refusals(dev):
    from viewformer_amd import ops
    img = torch.zeros((1, 8, 16, 3), dtype=torch.uint8, device=dev)
    for cout in (6, 1024):
        _refused(UNSUPPORTED, ops.conv_in, img, torch.zeros((cout, 3, 3, 3), device=dev), torch.zeros(cout, device=dev), 1, 8, 16, cout)
    for H, W, cout in ((12, 16, 128), (8, 24, 128), (8, 16, 64)):
        w = torch.zeros((128, 3, 3, 3), device=dev)
        _refused(UNSUPPORTED, ops.conv_in, torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev), w, torch.zeros(128, device=dev), 1, H, W, cout,
                 wp3h=ops.pack_conv_in_x3h(w))


@pytest.mark.parametrize('u8', [True, False], ids=['u8', 'f32'])
@pytest.mark.parametrize('row', K.CONV_IN_X3H_ROWS, ids=_id)
def test_conv_in_x3h_form(dev, row, u8):
    from viewformer_amd import ops
    n, H, W, cout = row
    img, w, b = K.conv_in_inputs((cout, n, H, W))
    ref, mag = K.conv_in_ref(img, w, b)
    src = img.to(dev) if u8 else K.preprocess_u8(img).to(dev)
    part = ops.new_gn_part(n, H, W, dev)
    part.fill_(float('nan'))
    o3 = ops.conv_in(src, w.to(dev), b.to(dev), n, H, W, cout, wp3h=ops.pack_conv_in_x3h(w.to(dev)), gn_part=part)
    ov = ops.conv_in(src, w.to(dev), b.to(dev), n, H, W, cout)
    (mx3, rms3), (mxv, rmsv) = _err(o3.cpu(), ref, mag), _err(ov.cpu(), ref, mag)
    _note('max:conv_in_x3h', mx3)
    _note('rms/f32:conv_in_x3h', rms3 / (rmsv + 1e-30))
    print(f'{row} u8={u8}: x3h max {mx3:.2e} rms {rms3:.2e} | VALU fp32 max {mxv:.2e} rms {rmsv:.2e}')
    assert mx3 < K.CONV_IN_X3H_MAX and rms3 < K.X6_RMS * rmsv + 1e-9
    assert bool(torch.isfinite(part).all()), 'a slot of the partial statistics was left unwritten'
    gamma = K.normal((cout,), 23, 0.3, 1.0)
    mean_f, scale_f = (t.double().cpu() for t in ops.groupnorm_finalize(part, gamma.to(dev), n, H * W, cout))
    mean_s, scale_s = CR.gn_stats64(o3.cpu().view(n * H * W, cout), gamma, n, H * W, cout)
    em = float((mean_f - mean_s).abs().max()) / (1 + float(mean_s.abs().max()))
    es = float(((scale_f - scale_s).abs() / scale_s.abs()).max())
    _note('gn mean:conv_in_x3h', em)
    _note('gn scale:conv_in_x3h', es)
    assert em < K.GN_MEAN_TOL and es < K.GN_SCALE_TOL, (em, es)


# ================================================================== conv3_small_cout
def _small(x, w, b, row, dev, bf16, pro=None, swish=True):
    from viewformer_amd import ops
    cin, cout, n, H, W = row
    xr = CR.to_rows(x).contiguous().to(dev)
    out = torch.full((n * H * W + 1, cout), -777.0, device=dev)
    ops.conv3_small_cout(xr.to(torch.bfloat16) if bf16 else xr, w.to(dev), None if b is None else b.to(dev), n, H, W, cin, cout,
                         pro=None if pro is None else tuple(None if t is None else t.to(dev) for t in pro), pro_swish=swish, out=out)
    torch.cuda.synchronize()
    assert bool((out[n * H * W:] == -777.0).all())
    return out[:n * H * W].cpu()


@pytest.mark.parametrize('bf16', [False, True], ids=['f32in', 'bf16in'])
@pytest.mark.parametrize('row', K.SMALL_ROWS, ids=_id)
def test_conv3_small_cout(dev, row, bf16):
    x, w, b, mc, sc, beta = K.small_inputs(row, bf16)
    fails = []
    for pro in K.SMALL_PRO:
        for bias in (b, None):
            p = None if pro is None else (mc, sc, beta)
            ref, mag, MAG = K.small_ref(x, w, bias, p, pro == 'swish')
            got = _small(x, w, bias, row, dev, bf16, pro=p, swish=pro == 'swish')
            ok, wst = K.within(got, ref, K.pro_bound(C['small'], mag, MAG, pro == 'swish', K.SWISH_1ULP_U))
            _note('small:error / bound' + (f' ({pro})' if pro else ''), wst)
            print(f'{row} bf16={bf16} pro={pro} bias={bias is not None}: worst {wst:.3f} of its bound (c = {C["small"]:g})')
            if not ok:
                fails.append(f'pro={pro} bias={bias is not None}: {wst:.3f} of its bound')
    xe, we, be = K.small_exact_inputs(row)
    bad = K.mismatches(_small(xe, we, be, row, dev, bf16), K.small_ref(xe, we, be, None, False)[0])
    _note('exact:conv3_small_cout', bad)
    if bad:
        fails.append(f'exact class: {bad} elements differ')
    assert not fails, f'{row} bf16={bf16}: ' + '; '.join(fails)


def test_conv3_small_cout_refusals(dev):
    for row in K.SMALL_REFUSED:
        cin, cout, n, H, W = row
        x, w = torch.zeros((n, cin, H, W)), torch.zeros((cout, cin, 3, 3))
        _refused(UNSUPPORTED, _small, x, w, None, row, dev, False)
    row = K.SMALL_ROWS[0]
    x, w, b, mc, sc, beta = K.small_inputs(row, False)
    for pro in ((None, sc, beta), (mc, None, beta), (mc, sc, None)):
        _refused(BAD_ARG, _small, x, w, b, row, dev, False, pro=pro)


# ================================================================== the codec's own activations against the variance rule
def test_full_size_codec_activations_stay_inside_the_variance_rule(dev, full_vq):
    """encode and decode of the golden images on the path VQGAN._gn takes: at every GroupNorm the activation is read back, mean^2 / var
    per (image, group) taken in float64, and the variance rule evaluated at the layer's largest ratio must stay below 1e-5"""
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import synthetic_scene_batch
    cfg, sd, g = full_vq
    m = VQGAN(cfg, data_format='NHWC').load_state_dict(sd).to(dev)
    frames, _ = synthetic_scene_batch(1, 4, 128, seed=int(g['input_seed']))
    layers, inner = [], m._gn

    def spy(x, name, n, HW, Cc, part=None):
        path = 'finalize' if part is not None else 'stats'
        xg = x.double().view(n, HW, 32, Cc // 32)
        mean, var = xg.mean(dim=(1, 3)), xg.var(dim=(1, 3), unbiased=False)
        out = inner(x, name, n, HW, Cc, part)
        rstd = 1.0 / torch.sqrt(var + K.EPS)
        got = out[1].double().view(n, 32, Cc // 32) / m._norm[name][0].double().view(1, 32, Cc // 32)
        rel = (got - rstd.unsqueeze(-1)).abs() / rstd.unsqueeze(-1)
        layers.append((name, path, HW, Cc, float((mean * mean / var).max()), float(K.rstd_bound(C['gn_var'], mean, var).max()),
                       float(rel[torch.isfinite(rel)].max())))
        return out
    m._gn = spy
    t0 = time.time()
    dec = m.decode_code(m.encode(torch.from_numpy(frames[0]).to(dev))[-1])
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert tuple(dec.shape) == (4, 128, 128, 3) and len(layers) >= 60
    for name, path, HW, Cc, ratio, bound, rel in layers:
        parity_report(test='codec_kernels', kernel=f'GroupNorm {name}', path=path, HW=HW, C=Cc, mean2_over_var=ratio, rule=bound, rstd_error=rel)
    worst = max(layers, key=lambda r: r[5])
    print(f'{len(layers)} GroupNorm layers in {dt:.2f} s (with the float64 read-back): largest mean^2 / var {max(r[4] for r in layers):.3f}, '
          f'largest bound {worst[5]:.2e} at {worst[0]}, largest measured rstd error {max(r[6] for r in layers):.2e}')
    assert all(r[5] < GN_CODEC_TOL for r in layers), [r for r in layers if not r[5] < GN_CODEC_TOL]
    assert all(r[6] <= r[5] for r in layers), [r for r in layers if not r[6] <= r[5]]
