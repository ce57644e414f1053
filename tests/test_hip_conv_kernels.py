"""GPU: the 3x3 convolution kernels one by one against the float64 reference of tests/conv_kernels_ref.py (pinned on the CPU by
tests/test_conv_kernels_ref_host.py), off the square, power-of-two path: non-square maps of one to four 8 x 16 tiles, Cin / 32 = 1, 2, 3,
5, 6, three 128-column blocks, absent bias / residual, strided output and residual, the weight gradient's slab sum and dX on its own.

Arms: 'f32' = vf_igemm_f32 (conv3_halo_f32.hip on stride-1 / upsample halo shapes, the per-tap kernel of igemm_f32.hip elsewhere: never
refuses), 'x6', 'x3h' (16x16x32 MFMAs where conv3_halo_x3h.hip::dispatch_pro picks them), 'x3h_k16' (SEL_CONV_X3H_K32 = 0: 32x32x16
everywhere), 'bf16', 'bf16_16' (bf16 activations in and out).  A row an arm does not take must raise VfError.

Exact class: integer activations, quarter-step weights: every arm returns the float64 reference as values, 0 differing elements
(bf16 out: the round-to-nearest-even bf16 of the exact value).
Rounded class: x6 / x3h hold the standing claim (max error < 6e-7 of magnitude, rms < 1.25 x the native f32 arm's + 1e-9); bf16 its standing
rule (reference on bf16-rounded operands, max |error| / max |reference| < 3e-5, 3e-3 behind the GroupNorm prologue); the native f32 arms,
the weight gradient's nine tap blocks + bias row and dX meet c x 2^-24 x magnitude per element with ``C`` below: 4 x the worst error of the
float32 CPU restatement on these very inputs (the host file's calibration), rounded up to a power of two, never a figure of the kernel.
Every kernel's worst figure goes to the parity report (profiles/conv_kernels_parity.txt)."""
import pytest
import torch

import conv_kernels_ref as R
from conftest import parity_report

pytestmark = pytest.mark.gpu

# c = 4 x basis rounded up to a power of two; basis = worst error of the float32 CPU restatement against float64 in units of
# 2^-24 x magnitude, as test_conv_kernels_ref_host.py measures and prints it (recorded in profiles/conv_kernels_parity.txt)
C = {
    'halo_f32': 16.0,              # basis 3.30
    'tap': 16.0,                   # basis 3.05
    'wgrad': 32.0,                 # basis 5.50
    'dx': 32.0,                    # basis 4.21
}

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
        parity_report(test='conv_kernels', kernel=k, worst=_worst[k], c=C.get(k, ''))


def _id(row):
    return '-'.join(str(v) for v in row)


def _launch(arm, row, xn, w, b, res, dev, pro=None, swish=True, gn_part=None, strided=False):
    """one launch of ``arm`` on NHWC rows ``xn`` [n Hin Win][Cin] (host tensors in, host tensor out: fp32, or bf16 for 'bf16_16');
    ``strided``: out / res are the first Cout columns of [M][Cout + 4] / [M][Cout + 8] buffers, the columns behind keep their sentinel"""
    from viewformer_amd import _lib, ops
    mode, cin, cout, H, W, n = row[:6]
    Ho, Wo = R.out_hw(mode, H, W)
    M = n * Ho * Wo
    a16 = arm == 'bf16_16'
    act = torch.bfloat16 if a16 else torch.float32
    wd = w.to(dev)
    wp = (ops.pack_conv_oihw(wd) if arm == 'f32' else ops.pack_conv3_x6(wd) if arm == 'x6' else
          ops.pack_conv3_bf16(wd) if arm in ('bf16', 'bf16_16') else ops.pack_conv3_x3h(wd))
    ldc, ldr = (cout + 4, cout + 8) if strided else (cout, cout)
    obuf = torch.full((M, ldc), -777.0, dtype=act, device=dev)
    rbuf = None
    if res is not None:
        rbuf = torch.full((M, ldr), 555.0, dtype=act, device=dev)
        rbuf[:, :cout] = res.to(dev).to(act)
    kw = dict(bias=None if b is None else b.to(dev), res=None if rbuf is None else rbuf[:, :cout], mode=R.MODE_ID[mode], pro=pro, pro_swish=swish,
              Hin=H, Win=W, Hout=Ho, Wout=Wo, ldc=ldc, ldr=ldr, gn_part=gn_part, x6=arm == 'x6', x3h=arm in ('x3h', 'x3h_k16'),
              bf16=arm in ('bf16', 'bf16_16'), a16=a16, o16=a16)
    prev = _lib.select(_lib.SEL_CONV_X3H_K32, 0 if arm == 'x3h_k16' else 1) if arm in ('x3h', 'x3h_k16') else None
    try:
        ops.igemm(xn.to(dev).to(act), wp, M, cin, cout, obuf[:, :cout], **kw)
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            _lib.select(_lib.SEL_CONV_X3H_K32, prev)
    assert bool((obuf[:, cout:] == -777.0).all()), f'{arm} {row}: columns behind Cout were written'
    return obuf[:, :cout].cpu()


def _refused(arm, row, xn, w, b, res, dev, **kw):
    from viewformer_amd import ops
    with pytest.raises(ops._lib.VfError):
        _launch(arm, row, xn, w, b, res, dev, **kw)


def _kernel_name(arm, row, **kw):
    return R.f32_kernel(row) if arm == 'f32' else 'x3h:' + R.x3h_kernel(row, k32=arm == 'x3h', **kw) if arm.startswith('x3h') else arm


def _exact(arm, row, got, ref, what=''):
    want = ref.float().to(torch.bfloat16) if arm == 'bf16_16' else ref
    bad = R.mismatches(got, want)
    _note('exact:' + _kernel_name(arm, row), bad)
    assert bad == 0, f'{arm} {row} {what}: {bad} of {want.numel()} elements differ from the reference'


# ------------------------------------------------------------------ exact class
@pytest.mark.parametrize('row', R.HALO_ROWS + R.TAP_ROWS, ids=_id)
def test_exact_class_every_arm_returns_the_reference(dev, row):
    x, w, b, res = R.exact_inputs(row)
    ref, _ = R.conv_ref(x, w, b, res, row[0])
    xn = R.to_rows(x).contiguous()
    for arm in R.ARMS:
        if R.arm_accepts(arm, row):
            _exact(arm, row, _launch(arm, row, xn, w, b, res, dev), ref)
        else:
            _refused(arm, row, xn, w, b, res, dev)


@pytest.mark.parametrize('variant', R.EPI_VARIANTS)
@pytest.mark.parametrize('row', R.EPI_ROWS, ids=_id)
def test_exact_class_epilogue_variants(dev, row, variant):
    """bias / residual absent, and out / res as the leading columns of wider buffers (ldc = Cout + 4, ldr = Cout + 8)"""
    x, w, b, res = R.exact_inputs(row)
    if variant in ('no_bias', 'neither'):
        b = None
    if variant in ('no_res', 'neither'):
        res = None
    ref, _ = R.conv_ref(x, w, b, res, row[0])
    xn = R.to_rows(x).contiguous()
    ran = 0
    for arm in R.ARMS:
        if R.arm_accepts(arm, row):
            _exact(arm, row, _launch(arm, row, xn, w, b, res, dev, strided=variant == 'strided'), ref, variant)
            ran += 1
    assert ran >= 1


# ------------------------------------------------------------------ rounded class
def _err(out, ref, mag):
    e = (out.double() - ref).abs() / mag
    return float(e.max()), float(e.pow(2).mean().sqrt())


@pytest.mark.parametrize('row,pro', R.ROUNDED_ROWS, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_rounded_class(dev, row, pro):
    from viewformer_amd import ops
    mode, cin, cout, H, W, n = row
    x, w, b, res, gamma, beta = R.rounded_inputs(row)
    xn = R.to_rows(x).contiguous()
    prol, a64 = None, x.double()
    if pro:
        # the reference applies the SAME fp32 statistics in fp64 so that only the prologue's and the convolution's arithmetic is compared
        if R.gn_stats_supported(cin):
            mean_c, scale_c = ops.groupnorm_stats(xn.to(dev), gamma.to(dev), n, H * W, cin)
        else:
            mean_c, scale_c = (t.to(dev) for t in R.gn_stats_f32(xn, gamma, n, H * W, cin))
        prol = (mean_c, scale_c, beta.to(dev))
        a64 = R.prologue(x, mean_c.cpu(), scale_c.cpu(), beta, pro == 'swish')
    ref, mag = R.conv_ref(a64, w, b, res, mode)
    kw = dict(pro=prol, swish=pro == 'swish')
    o32 = _launch('f32', row, xn, w, b, res, dev, **kw)
    k32 = R.f32_kernel(row)
    r32 = R.worst_ratio(o32, ref, mag)
    mx32, rms32 = _err(o32, ref, mag)
    _note(k32, r32)
    print(f'{row} pro={pro}: {k32} worst {r32:.2f} x 2^-24 x magnitude (c = {C[k32]:g}), rms {rms32:.2e}')
    fails = []
    if not r32 <= C[k32]:
        fails.append(f'{k32}: {r32:.2f} x 2^-24 x magnitude exceeds c = {C[k32]:g}')
    for arm in ('x6', 'x3h', 'x3h_k16'):
        if not R.arm_accepts(arm, row, pro=bool(pro)):
            _refused(arm, row, xn, w, b, res, dev, **kw)
            continue
        mx, rms = _err(_launch(arm, row, xn, w, b, res, dev, **kw), ref, mag)
        name = _kernel_name(arm, row, pro=bool(pro))
        _note('max:' + name, mx)
        _note('rms/f32:' + name, rms / (rms32 + 1e-30))
        print(f'{row} pro={pro}: {name} max {mx:.2e} rms {rms:.2e} | {k32} max {mx32:.2e} rms {rms32:.2e}')
        if not (mx < R.X6_MAX and rms < R.X6_RMS * rms32 + 1e-9):
            fails.append(f'{name}: max {mx:.2e} rms {rms:.2e} against f32 rms {rms32:.2e}')
    if R.arm_accepts('bf16', row, pro=bool(pro)):
        bf = lambda t: t.float().to(torch.bfloat16).double()                      # noqa: E731   operand rounding of the arm
        refb, _ = R.conv_ref(bf(a64), bf(w), b, res, mode)
        ob = _launch('bf16', row, xn, w, b, res, dev, **kw)
        rel = float((ob.double() - refb).abs().max() / refb.abs().max())
        _note('rel:bf16' + ('+pro' if pro else ''), rel)
        print(f'{row} pro={pro}: bf16 rel {rel:.2e}')
        if not rel < (R.BF16_REL_PRO if pro else R.BF16_REL):
            fails.append(f'bf16: rel {rel:.2e}')
    else:
        _refused('bf16', row, xn, w, b, res, dev, **kw)
    assert not fails, f'{row} pro={pro}: ' + '; '.join(fails)


# ------------------------------------------------------------------ fused statistics
@pytest.mark.parametrize('with_res', [True, False], ids=['res', 'no_res'])
@pytest.mark.parametrize('row', R.STATS_ROWS, ids=_id)
def test_fused_statistics_against_float64_of_the_stored_output(dev, row, with_res):
    """groupnorm_finalize(partials of the epilogue) vs the float64 statistics of the output read back; every slot written.  Without the
    residual (and without the bias) the epilogue takes its other store path (halo_common.h: vf_store_tile_stats<false>)"""
    from viewformer_amd import ops
    mode, cin, cout, H, W, n = row
    Ho, Wo = R.out_hw(mode, H, W)
    x, w, b, res, _, _ = R.rounded_inputs(row)
    if not with_res:
        b, res = None, None
    gamma = R.normal((cout,), R.row_seed(row) + 7, 0.3, 1.0)
    xn = R.to_rows(x).contiguous()
    ran = set()
    for arm in ('x6', 'bf16', 'x3h', 'x3h_k16'):
        part = ops.new_gn_part(n, Ho, Wo, dev)
        part.fill_(float('nan'))
        if not R.arm_accepts(arm, row, gn=True):
            _refused(arm, row, xn, w, b, res, dev, gn_part=part)
            continue
        out = _launch(arm, row, xn, w, b, res, dev, gn_part=part)
        assert bool(torch.isfinite(part).all()), f'{arm}: a slot was left unwritten'
        mean_f, scale_f = (t.double().cpu() for t in ops.groupnorm_finalize(part, gamma.to(dev), n, Ho * Wo, cout))
        mean_s, scale_s = R.gn_stats64(out, gamma, n, Ho * Wo, cout)
        em = float((mean_f - mean_s).abs().max()) / (1 + float(mean_s.abs().max()))
        es = float(((scale_f - scale_s).abs() / scale_s.abs()).max())
        name = _kernel_name(arm, row, gn=True)
        ran.add(name)
        _note('gn mean:' + name, em)
        _note('gn scale:' + name, es)
        print(f'{row} {name}: mean error {em:.2e} (bound {R.GN_MEAN_TOL:g}), scale error {es:.2e} (bound {R.GN_SCALE_TOL:g})')
        assert em < R.GN_MEAN_TOL and es < R.GN_SCALE_TOL, (arm, em, es)
        if name == _kernel_name(arm, row):            # (64 -> 1024 on x3h: the statistics move the launch to the other MFMA shape, other last bits)
            assert torch.equal(out, _launch(arm, row, xn, w, b, res, dev)), f'{arm}: the statistics changed the stored output'
    assert ran


def test_fused_statistics_are_refused_at_twelve_channels_per_group(dev):
    from viewformer_amd import ops
    row = R.STATS_REFUSED
    x, w, b, res = R.exact_inputs(row)
    xn = R.to_rows(x).contiguous()
    for arm in ('x6', 'bf16', 'x3h', 'x3h_k16', 'f32'):
        _refused(arm, row, xn, w, b, res, dev, gn_part=ops.new_gn_part(row[5], row[3], row[4], dev))


# ------------------------------------------------------------------ weight gradient
def _rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize('row', R.WGRAD_ROWS, ids=_id)
def test_weight_gradient_tap_by_tap(dev, row):
    """vf_conv3_wgrad_x6 with two slabs: each of the nine [Cin][Cout] tap blocks and the bias row against float64 autograd on its own"""
    from viewformer_amd import train_ops as T
    mode, cin, cout, H, W, n = row
    Ho, Wo = R.out_hw(mode, H, W)
    assert T.conv3_wgrad_splits(cin, cout, n * Ho * Wo) == 2 and T.conv3_wgrad_supported(cin, n, Ho, Wo)      # the slab sum is taken
    x, w, dy = R.grad_inputs(row)
    dW, db, _ = R.conv_grads(x, w, dy, mode)
    mW, mb, _ = R.conv_grads(x, w, dy, mode, absolute=True)
    got = T.conv3_wgrad(R.to_rows(x).contiguous().to(dev), dy.to(dev), n, H, W, cin, Ho, Wo, cout, R.MODE_ID[mode]).cpu()
    assert got.shape[0] >= 9 * cin + 1
    ratios = [R.worst_ratio(got[t * cin:(t + 1) * cin], dW[t], mW[t]) for t in range(9)] + [R.worst_ratio(got[9 * cin], db, mb)]
    _note('wgrad', max(ratios))
    print(f'{row}: tap blocks + bias worst ' + ' '.join(f'{r:.2f}' for r in ratios) + f' x 2^-24 x magnitude (c = {C["wgrad"]:g})')
    rw, rb = _rel(got[:9 * cin], dW.reshape(9 * cin, cout)), _rel(got[9 * cin], db)
    _note('wgrad whole-tensor rel', max(rw, rb))
    assert max(ratios) <= C['wgrad'], ratios
    assert rw < R.WGRAD_REL and rb < R.WGRAD_REL, (rw, rb)


# ------------------------------------------------------------------ dX
@pytest.fixture(scope='module')
def trainer(dev):
    import test_vqgan_train as V
    _, cfg, sd = V._tiny()
    return V._trainer(cfg, sd)


@pytest.mark.parametrize('row', R.DX_ROWS, ids=_id)
def test_conv_dx_alone(dev, trainer, row):
    """VQGANTrainer._conv_dx (rotated weight, zero insertion for stride 2, padded reduction for cout % 32 != 0, upsample2_bwd) vs autograd"""
    mode, cin, cout, H, W, n = row
    Ho, Wo = R.out_hw(mode, H, W)
    x, w, dy = R.grad_inputs(row)
    _, _, dX = R.conv_grads(x, w, dy, mode)
    _, _, mX = R.conv_grads(x, w, dy, mode, absolute=True)
    got = trainer._conv_dx(w.to(dev), dy.to(dev), n, H, W, Ho, Wo, R.MODE_ID[mode]).cpu()
    assert got.shape == dX.shape
    r = R.worst_ratio(got, dX, mX)
    _note('dx', r)
    print(f'{row}: dX worst {r:.2f} x 2^-24 x magnitude (c = {C["dx"]:g})')
    assert r <= C['dx']
