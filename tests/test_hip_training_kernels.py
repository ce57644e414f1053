"""GPU: the small kernels under the codebook (VQGAN) trainer, the LPIPS loss and the transformer trainer's loss / clip path, one by one
against the float64 references of tests/training_kernels_ref.py (pinned on the CPU by tests/test_training_kernels_ref_host.py).

Exact class (copies, selections, sums of at most four terms): inputs on a dyadic grid (multiples of 2^-6 in [-8, 8], planted ties, exact
zeros, -0.0), every fp32 operation is exact and the result must equal the reference as values, element for element (-0 == +0).
Rounded class: |got - want| <= c x 2^-24 x magnitude per element, the magnitude being the reference expression with every summand
replaced by its absolute value.  ``C`` below holds one constant per kernel: 4 x the worst error the float32 CPU restatement of the kernel
shows against float64 on these very inputs (the host file's calibration; the factor covers another valid summation order and expf),
rounded up to a power of two — never a figure taken from the kernel.  A lost term, a stale tail or a wrong tie lands at 1e-3 of the
magnitude, four orders above.  Every kernel's measured worst ratio goes to the parity report (profiles/training_kernels_parity.txt).

Shapes are the smallest at which each property can fail.  Where an entry point refuses a listed shape the nearest accepted one is used:
  * ops.groupnorm_stats takes power-of-two channel counts only (C / 4 divides 256): for C = 96 and 320 the backward — which accepts them —
    is handed the float32 rounding of the float64 statistics (training_kernels_ref.gn_stats_f32), and the zero-gain case runs a second
    time at C = 128 on the statistics kernel's own output.
  * a maximum pool or an upsample backward of more than 16384 x 256 / 8192 x 256 work items, the ReLU of 4 (16384 x 256) + 4 elements and
    the LPIPS head of more than 4 x 65536 pixels are compared on the device: inputs drawn there, the same float64 torch statement run
    there (selections and four-term sums of dyadic numbers are exact in any precision).
"""
import ctypes

import numpy as np
import pytest
import torch

import training_kernels_ref as R
from conftest import parity_report

pytestmark = pytest.mark.gpu

# c per kernel = 4 x basis, rounded up to a power of two; basis = worst error of the float32 CPU restatement against float64 in units of
# 2^-24 x magnitude, as test_training_kernels_ref_host.py measures and prints it (recorded in profiles/training_kernels_parity.txt).
# groupnorm_bwd: 32 as specified with the test (basis 6.9 over four shapes then; 3.8 with this file's magnitudes).
C = {
    'lpips_scaling': 8.0,          # basis 1.83
    'groupnorm_bwd': 32.0,
    'softmax_rows_bwd_': 16.0,     # basis 3.72
    'lpips_head': 8.0,             # basis 1.15
    'lpips_head_bwd': 32.0,        # basis 5.70
    'pose_mse': 16.0,              # basis 3.41
    'dense_small_k_bwd': 32.0,     # basis 4.18
    'clip_by_norm_': 4.0,          # basis 0.74
    'clip_grad_norm_': 4.0,        # basis 0.53
    'l1_loss': 4.0,                # basis 0.95
}

BAD_ARG, UNSUPPORTED = -1, -2
_worst = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        parity_report(test='training_kernels', kernel=k, worst_ratio=_worst[k], c=C.get(k, 0.0),
                      unit='2^-24 x magnitude' if k in C else 'mismatching elements')


def _lib_():
    from viewformer_amd import _lib
    return _lib.load()


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _exact(kernel, got, want, what=''):
    bad = R.mismatches(got.to(want.device) if torch.is_tensor(got) else got, want)
    _worst[kernel] = max(_worst.get(kernel, 0), bad)
    assert bad == 0, f'{kernel} {what}: {bad} elements differ from the reference'


def _close(kernel, got, want, mag, what=''):
    r = R.worst_ratio(got.to(R.t64(want).device), want, mag)
    _worst[kernel] = max(_worst.get(kernel, 0.0), r)
    print(f'{kernel} {what}: worst {r:.3f} x 2^-24 x magnitude (c = {C[kernel]:g})')
    assert r <= C[kernel], f'{kernel} {what}: {r:.3f} x 2^-24 x magnitude exceeds c = {C[kernel]:g}'


def _dyadic_dev(n, seed, dev):
    """the dyadic grid drawn on the device (largest cases): multiples of 2^-6 in [-8, 8]; every 16th element zero, every 17th -0.0, every
    fifth equal to its predecessor"""
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randint(-512, 513, (n,), generator=g, device=dev).to(torch.float32) / 64.0
    a[::16] = 0.0
    a[::17] = -0.0
    i = torch.arange(5, n, 5, device=dev)
    a[i] = a[i - 1]
    return a


# ------------------------------------------------------------------ exact class
def test_gather_transpose(dev):
    """P = 105 / 36 and C = 45 are no multiples of the 32 x 32 tile; stride 2 with Hout = ceil(Hin / 2) reads past the right / bottom edge as
    zero; a destination with ld > P keeps its sentinel in the columns from P on"""
    from viewformer_amd import train_ops as T
    n, Hin, Win, Cc = 3, 5, 7, 45
    x = R.dyadic((n, Hin, Win, Cc), 201)
    xd = x.to(dev)
    for stride, offs, (Hout, Wout) in ((1, (-1, 0, 1), (Hin, Win)), (2, (0, 1, 2), ((Hin + 1) // 2, (Win + 1) // 2))):
        for oy in offs:
            for ox in offs:
                want, _ = R.gather_transpose(x, n, Hin, Win, Cc, Hout, Wout, stride, oy, ox)
                got = T.gather_transpose(xd.view(-1, Cc), n, Hin, Win, Cc, Hout, Wout, stride, oy, ox)
                _exact('gather_transpose', got.cpu(), want, f'stride {stride} ({oy},{ox})')
    P, ld = n * Hin * Win, n * Hin * Win + 11
    dst = torch.full((Cc, ld), -777.0, device=dev)
    st = _lib_().vf_gather_transpose_f32(_P(xd), _P(dst), n, Hin, Win, Cc, Hin, Win, 1, 1, -1, ld, _strm())
    assert st == 0
    want, _ = R.gather_transpose(x, n, Hin, Win, Cc, Hin, Win, 1, 1, -1)
    _exact('gather_transpose', dst[:, :P].cpu(), want, 'ld > P')
    assert bool((dst[:, P:] == -777.0).all()), 'columns from P on were written'
    assert _lib_().vf_gather_transpose_f32(_P(xd), _P(dst), n, Hin, Win, Cc, Hin, Win, 1, 0, 0, P - 1, _strm()) == BAD_ARG


@pytest.mark.parametrize('shape', [(1, 1, 1, 4), (3, 5, 7, 12), (1, 1024, 1026, 8)])
def test_upsample2_bwd(dev, shape):
    """the last shape has n H W C / 4 = 2 101 248 > 8192 x 256: the grid-stride loop runs a second lap"""
    from viewformer_amd import train_ops as T
    n, H, W, Cc = shape
    big = n * H * W * Cc > 1 << 20
    du = _dyadic_dev(n * 4 * H * W * Cc, 210, dev) if big else R.dyadic((n * 4 * H * W * Cc,), 210 + H)
    got = T.upsample2_bwd(du.to(dev).view(-1, Cc), n, H, W, Cc)
    _exact('upsample2_bwd', got, R.upsample2_bwd(du, n, H, W, Cc)[0], str(shape))
    dx = torch.empty((n * H * W, 6), device=dev)
    assert _lib_().vf_upsample2_bwd_f32(_P(du.to(dev)), _P(dx), 1, 1, 1, 6, _strm()) == BAD_ARG


@pytest.mark.parametrize('n', [4, 1028, 4 * (16384 * 256) + 4])
def test_relu_and_its_backward(dev, n):
    """zeros of both signs and the smallest positive normal among the inputs; n = 6 (no multiple of 4) is refused"""
    from viewformer_amd import train_ops as T
    x = _dyadic_dev(n, 220, dev) if n > 1 << 20 else R.dyadic((n,), 220 + n).to(dev)
    x[0], x[1], x[2], x[3] = 0.0, -0.0, float(np.finfo(np.float32).tiny), -float(np.finfo(np.float32).tiny)
    dy = _dyadic_dev(n, 221, dev) if n > 1 << 20 else R.dyadic((n,), 221 + n, ties=False).to(dev)
    dy[:4] = 1.5
    src = x if n > 1 << 20 else x.cpu()
    y = T.relu_(x.clone())
    _exact('relu_', y, R.relu(src)[0], f'n {n}')
    assert float(y[2]) == float(np.finfo(np.float32).tiny) and float(y[3]) == 0.0
    g = T.relu_bwd_(dy.clone(), y)
    _exact('relu_bwd_', g, R.relu_bwd(dy if n > 1 << 20 else dy.cpu(), R.relu(src)[0])[0], f'n {n}')
    assert g[:4].tolist() == [0.0, 0.0, 1.5, 0.0]
    six = torch.ones(8, device=dev)
    assert _lib_().vf_relu_f32(_P(six), 6, _strm()) == BAD_ARG and _lib_().vf_relu_bwd_f32(_P(six), _P(six), 6, _strm()) == BAD_ARG
    assert bool((six == 1.0).all())


def _plant_ties(x, n, H, W, Cc):
    """windows with all four values equal and with the maximum twice, at positions (0, 1), (1, 2), (2, 3) of the row-major window"""
    v = x.view(n, H, 2, W, 2, Cc)
    cells = [(h, w) for h in range(H) for w in range(W)]
    v[0, cells[0][0], :, cells[0][1], :, :] = 2.0
    for k, pair in enumerate(((0, 1), (1, 2), (2, 3))):
        if k + 1 < len(cells):
            h, w = cells[k + 1]
            for p in pair:
                v[0, h, p // 2, w, p % 2, :] = 8.5                                # above every grid value but 8: a shared maximum
            v[0, h, :, w, :, 0] = 8.5                                             # channel 0: all four at the maximum
    return x


@pytest.mark.parametrize('shape', [(1, 1, 1, 4), (2, 3, 5, 12), (2, 3, 5, 3), (2, 129, 128, 128)])
def test_maxpool2_and_its_backward(dev, shape):
    """C = 3 for the backward only (the forward works in float4); the last shape has n Hout Wout C = 4 227 072 > 16384 x 256 (the backward's
    second lap; the forward's second lap has a test of its own below).  Ties: the gradient goes to the first
    maximum in row-major order, as F.max_pool2d sends it"""
    from viewformer_amd import train_ops as T
    n, H, W, Cc = shape
    big = n * H * W * Cc > 1 << 20
    x = _dyadic_dev(n * 4 * H * W * Cc, 230, dev) if big else R.dyadic((n * 4 * H * W * Cc,), 230 + Cc)
    x = _plant_ties(x, n, H, W, Cc)
    dy = (_dyadic_dev(n * H * W * Cc, 231, dev) if big else R.dyadic((n * H * W * Cc,), 231 + Cc, ties=False)) + 0.0078125      # never zero
    xd, dyd = x.to(dev), dy.to(dev)
    if Cc % 4 == 0:
        _exact('maxpool2', T.maxpool2(xd.view(-1, Cc), n, H, W, Cc), R.maxpool2(x, n, H, W, Cc)[0], str(shape))
    else:
        assert _lib_().vf_maxpool2_f32(_P(xd), _P(torch.empty(n * H * W * Cc, device=dev)), n, H, W, Cc, _strm()) == BAD_ARG
    got = T.maxpool2_bwd(xd.view(-1, Cc), dyd.view(-1, Cc), n, H, W, Cc)
    _exact('maxpool2_bwd', got, R.maxpool2_bwd(x, dy, n, H, W, Cc)[0], str(shape))
    v = got.view(n, H, 2, W, 2, Cc)
    assert float(v[0, 0, 0, 0, 0, 0]) == float(dyd.view(n, H, W, Cc)[0, 0, 0, 0]) and float(v[0, 0, :, 0, :, 0].abs().sum()) == abs(float(v[0, 0, 0, 0, 0, 0]))


def test_maxpool2_second_lap(dev):
    """n Hout Wout C / 4 = 4 202 496 > 16384 x 256: the forward's grid-stride loop comes round (input and reference on the device)"""
    from viewformer_amd import train_ops as T
    n, H, W, Cc = 1, 1026, 1024, 16
    x = _plant_ties(_dyadic_dev(n * 4 * H * W * Cc, 232, dev), n, H, W, Cc)
    _exact('maxpool2', T.maxpool2(x.view(-1, Cc), n, H, W, Cc), R.maxpool2(x, n, H, W, Cc)[0], str((n, H, W, Cc)))


@pytest.mark.parametrize('n', R.L1_SIZES)
def test_l1_loss(dev, n):
    """dy exact (0 where x == y: a tenth of the elements), the sum rounded; 1024 x 2048 + 1 elements is past the cap of 1024 partials"""
    from viewformer_amd import train_ops as T
    x, y = R.l1_inputs(n)
    (want, wdy), (mag, _) = R.l1_loss(x, y, 0.25)
    total, dy = T.l1_loss(x.to(dev), y.to(dev), 0.25)
    _exact('l1_loss dy', dy.cpu(), wdy, f'n {n}')
    assert int((dy == 0).sum()) >= (n + 9) // 10
    _close('l1_loss', total.cpu().view(1), want.view(1), mag.view(1), f'n {n}')
    assert int(_lib_().vf_l1_loss_partials(n)) == min(1024, (n + 2047) // 2048)


@pytest.mark.parametrize('n', [1, 1028, 8192 * 256 + 5])
def test_axpby_and_add(dev, n):
    from viewformer_amd import train_ops as T
    x, y = R.dyadic((n,), 240 + n % 7), R.dyadic((n,), 241 + n % 7)
    xd, yd = x.to(dev), y.to(dev)
    _exact('axpby', T.axpby(1.25, xd, -0.375, yd).cpu(), R.axpby(1.25, x, -0.375, y)[0], f'n {n}')
    _exact('axpby', T.axpby(-2.5, xd).cpu(), R.axpby(-2.5, x)[0], f'n {n}, y = None')
    alias = xd.clone()
    assert T.axpby(0.5, alias, out=alias) is alias                                       # as lpips.py / vqgan_train.py call it
    _exact('axpby', alias.cpu(), R.axpby(0.5, x)[0], f'n {n}, out = x')
    alias = yd.clone()
    T.axpby(1.25, xd, -0.375, alias, out=alias)
    _exact('axpby', alias.cpu(), R.axpby(1.25, x, -0.375, y)[0], f'n {n}, out = y')
    _exact('add_', T.add_(xd.clone(), yd).cpu(), R.axpby(1.0, x, 1.0, y)[0], f'n {n}')


def test_axpby_and_add_of_nothing_leave_the_output_untouched(dev):
    out = torch.full((4,), -777.0, device=dev)
    x = torch.ones(4, device=dev)
    assert _lib_().vf_axpby_f32(2.0, _P(x), 0.0, None, _P(out), 0, _strm()) == 0
    assert _lib_().vf_add_inplace_f32(_P(out), _P(x), 0, _strm()) == 0
    assert bool((out == -777.0).all())


# ------------------------------------------------------------------ rounded class
@pytest.mark.parametrize('npix', R.SCALING_NPIX)
def test_lpips_scaling(dev, npix):
    """forward and backward; above 16384 x 256 / 3 pixels the loop laps and the channel of element i stays i mod 3"""
    from viewformer_amd import train_ops as T
    x = R.normal((npix * 3,), 20 + npix % 1000)
    for bwd in (False, True):
        want, mag = R.lpips_scaling(x, R.SHIFT3, R.SCALE3, bwd)
        _close('lpips_scaling', T.lpips_scaling(x.to(dev), R.SHIFT3, R.SCALE3, backward=bwd).cpu(), want, mag, f'npix {npix} bwd {bwd}')


def _gn_run(dev, x, da, mean_c, scale_c, gamma, beta, n, HW, Cc, groups, swish, dx0):
    """through _lib with accumulate = 1 on a non-zero dx"""
    from viewformer_amd import train_ops as T
    lib = _lib_()
    dx = dx0.to(dev).clone()
    chan = torch.empty((n, Cc, 2), device=dev)
    ws = torch.empty(int(lib.vf_groupnorm_bwd_workspace_bytes(n, HW, Cc, groups)), dtype=torch.uint8, device=dev)
    st = lib.vf_groupnorm_bwd_f32(_P(x), _P(da), _P(mean_c), _P(scale_c), _P(gamma), _P(beta), _P(dx), _P(chan), n, HW, Cc, groups, 1e-6,
                                  1 if swish else 0, 1, _P(ws), _strm())
    assert st == 0
    return dx


def _gn_check(dev, n, HW, Cc, groups, zero, gpu_stats, tag):
    from viewformer_amd import ops
    from viewformer_amd import train_ops as T
    x, da, gamma, beta, dx0 = R.gn_inputs(n, HW, Cc, groups, zero)
    xd, dad, gd, bd = x.to(dev), da.to(dev), gamma.to(dev), beta.to(dev)
    if gpu_stats:
        mean_c, scale_c = ops.groupnorm_stats(xd, gd, n, HW, Cc, groups, 1e-6)
    else:
        mean_c, scale_c = (t.to(dev) for t in R.gn_stats_f32(x, gamma, n, HW, Cc, groups)[:2])
    for swish in (False, True):
        (wdx, wdg, wdb), (mdx, mdg, mdb) = R.groupnorm_bwd(x, da, gamma, beta, n, HW, Cc, groups, swish)
        dx, dg, db = T.groupnorm_bwd(xd, dad, mean_c, scale_c, gd, bd, n, HW, Cc, swish, groups=groups)
        for nm, t in (('dx', dx), ('dgamma', dg), ('dbeta', db)):
            assert bool(torch.isfinite(t).all()), f'groupnorm_bwd {tag} swish {swish}: {nm} has {int((~torch.isfinite(t)).sum())} non-finite elements'
        _close('groupnorm_bwd', dx.cpu(), wdx, mdx, f'{tag} swish {swish} dx')
        _close('groupnorm_bwd', dg.cpu(), wdg, mdg, f'{tag} swish {swish} dgamma')
        _close('groupnorm_bwd', db.cpu(), wdb, mdb, f'{tag} swish {swish} dbeta')
        (adx, _, _), (amdx, _, _) = R.groupnorm_bwd(x, da, gamma, beta, n, HW, Cc, groups, swish, dx0=dx0)
        _close('groupnorm_bwd', _gn_run(dev, xd, dad, mean_c, scale_c, gd, bd, n, HW, Cc, groups, swish, dx0).cpu(), adx, amdx,
               f'{tag} swish {swish} dx accumulated')


@pytest.mark.parametrize('shape', R.GN_SHAPES)
def test_groupnorm_bwd(dev, shape):
    n, HW, Cc, groups = shape
    _gn_check(dev, n, HW, Cc, groups, False, (Cc // 4) > 0 and 256 % (Cc // 4) == 0, str(shape))


@pytest.mark.parametrize('Cc', [96, 128])
def test_groupnorm_bwd_with_zero_and_tiny_gains(dev, Cc):
    """gamma[1] = 0, gamma[C-2] = 1e-30 and one whole group of zero gains (pruned or zero-initialised gains occur in checkpoints): every
    output finite and within the bound of the other cases.  C = 96: the listed case, statistics rounded from float64; C = 128: the same
    on ops.groupnorm_stats' own output"""
    _gn_check(dev, 2, 100, Cc, 32, True, Cc == 128, f'zero gains C {Cc}')


def test_groupnorm_bwd_refuses_more_than_1024_channels(dev):
    t = torch.zeros(1056 * 4, device=dev)
    assert _lib_().vf_groupnorm_bwd_f32(_P(t), _P(t), _P(t), _P(t), _P(t), _P(t), _P(t), _P(t), 1, 1, 1056, 32, 1e-6, 0, 0, _P(t), _strm()) == UNSUPPORTED


@pytest.mark.parametrize('rows', [1, 5, 1027])
def test_softmax_rows_bwd(dev, rows):
    from viewformer_amd import train_ops as T
    for r, n in R.SOFTMAX_CASES:
        if r != rows:
            continue
        p, dp = R.softmax_inputs(rows, n)
        for scale in (1.0, 0.125):
            want, mag = R.softmax_rows_bwd(p, dp, scale)
            got = T.softmax_rows_bwd_(p.to(dev), dp.to(dev).clone(), rows, n, scale)
            _close('softmax_rows_bwd_', got.cpu(), want, mag, f'rows {rows} n {n} scale {scale}')


@pytest.mark.parametrize('n_img', [1, 3])
def test_lpips_head_and_its_backward(dev, n_img):
    """features after a ReLU; one pixel with f1 == 0 (k = 0 by the kernel's stated convention, which the reference states too: autograd
    gives NaN there) and one with f0 == f1 == 0; accumulate 0 and 1, gscale != 1"""
    from viewformer_amd import train_ops as T
    for n, HW, Cc in R.HEAD_CASES:
        if n != n_img:
            continue
        f0, f1, w, df0 = R.head_inputs(n, HW, Cc)
        a, b, wd = f0.to(dev), f1.to(dev), w.to(dev)
        want, mag = R.lpips_head(f0, f1, w, n, HW, Cc)
        _close('lpips_head', T.lpips_head(a, b, wd, n, HW, Cc).cpu(), want, mag, f'n {n} HW {HW} C {Cc}')
        for acc in (False, True):
            want, mag = R.lpips_head_bwd(f0, f1, w, df0, n * HW, Cc, 0.37, acc)
            got = T.lpips_head_bwd(a, b, wd, df0.to(dev).clone(), n * HW, Cc, 0.37, acc)
            _close('lpips_head_bwd', got.cpu(), want, mag, f'n {n} HW {HW} C {Cc} accumulate {acc}')


def test_lpips_head_backward_second_lap(dev):
    """npix > 4 x 65536 at C = 64: the backward's grid-stride loop comes round (compared on the device)"""
    from viewformer_amd import train_ops as T
    n, HW, Cc = R.HEAD_BIG
    g = torch.Generator(device=dev).manual_seed(5)
    f0 = torch.randn((HW, Cc), generator=g, device=dev).clamp_min(0)
    f1 = (f0 + 0.3 * torch.randn((HW, Cc), generator=g, device=dev)).clamp_min(0)
    w = 0.5 * torch.randn((Cc,), generator=g, device=dev)
    df0 = torch.randn((HW, Cc), generator=g, device=dev)
    f1[0] = 0.0
    f0[-1] = 0.0
    f1[-1] = 0.0
    want, mag = R.lpips_head_bwd(f0, f1, w, df0, HW, Cc, 0.37, True)
    _close('lpips_head_bwd', T.lpips_head_bwd(f0, f1, w, df0.clone(), HW, Cc, 0.37, True), want, mag, f'npix {HW} accumulate True')
    want, mag = R.lpips_head(f0, f1, w, n, HW, Cc)
    _close('lpips_head', T.lpips_head(f0, f1, w, n, HW, Cc), want, mag, f'HW {HW}')


@pytest.mark.parametrize('rows,L', R.POSE_CASES)
def test_pose_mse(dev, rows, L):
    """gt row = r // L; zero weights; w_ori distinct from row_weight; xyz_div None and given"""
    from viewformer_amd import train_ops as T
    raw, gt, wp, wo, div = R.pose_inputs(rows, L)
    for dv in (None, div):
        want, mag = R.pose_mse(raw, gt, wp, wo, dv, rows, L, 0.2)
        got = T.pose_mse(raw.to(dev), gt.to(dev), wp.to(dev), rows, L, 0.2, w_ori=wo.to(dev), xyz_div=None if dv is None else dv.to(dev))
        for nm, g, w_, m in zip(('pos', 'ori', 'draw'), got, want, mag):
            _close('pose_mse', g.cpu(), w_, m, f'rows {rows} L {L} div {dv is not None} {nm}')
    want, mag = R.pose_mse(raw, gt, wp, wp, None, rows, L, 0.2)
    _close('pose_mse', T.pose_mse(raw.to(dev), gt.to(dev), wp.to(dev), rows, L, 0.2)[2].cpu(), want[2], mag[2], f'rows {rows} L {L} w_ori default')


@pytest.mark.parametrize('rows,K,N', R.DENSE_CASES)
def test_dense_small_k_bwd(dev, rows, K, N):
    """dW and db start non-zero: the kernel adds into them"""
    from viewformer_amd import train_ops as T
    x, dy, dW0, db0 = R.dense_inputs(rows, K, N)
    (wW, wb), (mW, mb) = R.dense_small_k_bwd(x, dy, dW0, db0, rows, K, N)
    dW, db = dW0.to(dev).clone(), db0.to(dev).clone()
    T.dense_small_k_bwd(x.to(dev), dy.to(dev), dW, db, rows, K, N)
    _close('dense_small_k_bwd', dW.cpu(), wW, mW, f'({rows},{K},{N}) dW')
    _close('dense_small_k_bwd', db.cpu(), wb, mb, f'({rows},{K},{N}) db')
    assert _lib_().vf_dense_small_k_bwd_f32(_P(dW), _P(dW), _P(dW), _P(db), 1, 17, 1, _strm()) == UNSUPPORTED


@pytest.mark.parametrize('n', R.CLIP_SIZES)
def test_clip_by_norm_and_clip_grad_norm(dev, n):
    """both semantics (clip / max(norm, clip); max / (norm + 1e-6) only when below 1) below and above the limit; below it clip_grad_norm_
    leaves every bit; the all-zero vector stays zero"""
    from viewformer_amd import train_ops as T
    x = R.clip_input(n)
    norm = float(x.double().norm())
    sc = T.clip_scratch(dev)
    assert sc.numel() == int(_lib_().vf_clip_scratch_floats()) >= 1
    for lim in (0.5 * norm, 2.0 * norm):
        want, mag = R.clip_by_norm(x, lim)
        _close('clip_by_norm_', T.clip_by_norm_(x.to(dev).clone(), lim, sc).cpu(), want, mag, f'n {n} limit {lim / norm:.1f} norm')
        want, mag = R.clip_grad_norm(x, lim)
        got = T.clip_grad_norm_(x.to(dev).clone(), lim, sc).cpu()
        _close('clip_grad_norm_', got, want, mag, f'n {n} limit {lim / norm:.1f} norm')
        if lim > norm:
            assert torch.equal(got.view(torch.int32), x.view(torch.int32)), 'below the limit every bit stays'
    z = torch.zeros(n, device=dev)
    for f in (T.clip_by_norm_, T.clip_grad_norm_):
        out = f(z.clone(), 1.0, sc)
        assert bool((out == 0).all()) and bool(torch.isfinite(out).all())
    with pytest.raises(Exception):
        T.clip_grad_norm_(x.to(dev).clone(), 1.0, torch.zeros(1, device=dev))          # the one-float scratch of the earlier contract


# ------------------------------------------------------------------ the clip factor scales every gradient: its bits must not depend on scheduling
def test_clipping_is_bit_reproducible(dev):
    """50 calls of each entry point on the same 3 x 2^20 + 3 elements, a GEMM between the calls (tests/test_hip_repro.py::_repeat)"""
    from viewformer_amd import train_ops as T
    from test_hip_repro import _repeat
    x = R.clip_input(R.CLIP_SIZES[-1]).to(dev)
    lim = 0.5 * float(x.double().norm())
    sc = T.clip_scratch(dev)
    _repeat(lambda: (T.clip_by_norm_(x.clone(), lim, sc),), 50, 'clip_by_norm_')
    _repeat(lambda: (T.clip_grad_norm_(x.clone(), lim, sc),), 50, 'clip_grad_norm_')


def test_two_clipped_codebook_trainers_agree_bit_for_bit(dev):
    """two VQGANTrainers from the same weights, two steps each with gradient_clip_val below the gradient norm: identical flat_p"""
    from oracle import vqgan_oracle as vq
    from test_vqgan_train import _tiny, _trainer
    g, cfg, sd = _tiny()
    x = vq.preprocess_u8(torch.from_numpy(g['frames']))
    probe = _trainer(cfg, sd)
    probe.train_step(x, apply_update=False)
    cfg.gradient_clip_val = 0.5 * float(probe.flat_g.double().norm())                    # the clip is live on the first step
    assert cfg.gradient_clip_val > 0
    ps = []
    for _ in range(2):
        tr = _trainer(cfg, sd)
        tr.train_step(x)
        tr.train_step(x)
        torch.cuda.synchronize()
        ps.append(tr.flat_p.clone())
    assert torch.equal(ps[0].view(torch.int32), ps[1].view(torch.int32))
