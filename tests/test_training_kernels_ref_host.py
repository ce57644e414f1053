"""CPU: the float64 references of tests/training_kernels_ref.py pinned against independent float64 statements (torch.nn.functional
autograd, torch.nn.utils.clip_grad_norm_, oracle/lpips_oracle.py), the comparison helper checked against the ways kernels go wrong, and
the calibration that the constants of tests/test_hip_training_kernels.py come from: a float32 CPU restatement of every rounded kernel
against float64 on the GPU test's own inputs, in units of 2^-24 x magnitude."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import training_kernels_ref as R

F64 = torch.float64


def _same(a, b, tol=1e-12):
    a, b = R.t64(a), R.t64(b)
    return a.shape == b.shape and float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------ 1. pins
@pytest.mark.parametrize('stride,oy,ox', [(1, -1, 1), (1, 0, 0), (1, 1, -1), (2, 0, 0), (2, 1, 2), (2, 2, 1)])
def test_gather_is_the_operand_of_the_convolution_weight_gradient(stride, oy, ox):
    """dW[tap] = gather(tap) . dY, against F.conv2d autograd: stride 1 pads by one (tap offset ky - 1), stride 2 pads right / bottom (an even
    image, as the Downsample layer sees it: Hout = Hin / 2 and the last taps read the padding)"""
    n, Hin, Win, C, Co = (3, 5, 7, 5, 4) if stride == 1 else (3, 6, 8, 5, 4)
    x = R.dyadic((n, Hin, Win, C), 1).double()
    w = torch.zeros((Co, C, 3, 3), dtype=F64, requires_grad=True)
    xn = x.permute(0, 3, 1, 2)
    y = F.conv2d(xn, w, padding=1) if stride == 1 else F.conv2d(F.pad(xn, (0, 1, 0, 1)), w, stride=2)
    Hout, Wout = y.shape[2], y.shape[3]
    assert (Hout, Wout) == ((Hin, Win) if stride == 1 else ((Hin + 1) // 2, (Win + 1) // 2))
    dy = R.normal((n, Co, Hout, Wout), 2).double()
    y.backward(dy)
    ky, kx = (oy + 1, ox + 1) if stride == 1 else (oy, ox)
    dst, _ = R.gather_transpose(x, n, Hin, Win, C, Hout, Wout, stride, oy, ox)
    assert _same(dst @ dy.permute(0, 2, 3, 1).reshape(-1, Co), w.grad[:, :, ky, kx].t())


def test_upsample_and_maxpool_against_functional():
    n, H, W, C = 3, 5, 7, 12
    du = R.dyadic((n, 2 * H, 2 * W, C), 3).double()
    x = torch.zeros((n, C, H, W), dtype=F64, requires_grad=True)
    (F.interpolate(x, scale_factor=2.0, mode='nearest') * du.permute(0, 3, 1, 2)).sum().backward()
    assert R.mismatches(R.upsample2_bwd(du, n, H, W, C)[0], x.grad.permute(0, 2, 3, 1).reshape(-1, C)) == 0
    xi = R.dyadic((n, 2 * H, 2 * W, C), 4)
    xi.view(n, H, 2, W, 2, C)[0, 0, :, 0, :, :] = 1.5                         # all four equal
    xi.view(n, H, 2, W, 2, C)[0, 1, 0, 1, :, :] = 9.0                         # a tie at positions (0, 1)
    xn = xi.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.max_pool2d(xn, 2)
    dy = R.dyadic((n, H, W, C), 5).double()
    y.backward(dy.permute(0, 3, 1, 2))
    assert R.mismatches(R.maxpool2(xi, n, H, W, C)[0], y.detach().permute(0, 2, 3, 1).reshape(-1, C)) == 0
    assert R.mismatches(R.maxpool2_bwd(xi, dy, n, H, W, C)[0], xn.grad.permute(0, 2, 3, 1).reshape(-1, C)) == 0


def test_relu_l1_axpby_against_functional():
    x = R.dyadic((1028,), 6)
    xd = x.double().clone().requires_grad_(True)
    y = F.relu(xd)
    dy = R.dyadic((1028,), 7).double()
    y.backward(dy)
    assert R.mismatches(R.relu(x)[0], y.detach()) == 0 and R.mismatches(R.relu_bwd(dy, y.detach())[0], xd.grad) == 0
    a, b = R.l1_inputs(2049)
    bd = b.double().clone().requires_grad_(True)
    s = F.l1_loss(bd, a.double(), reduction='sum')
    (0.25 * s).backward()
    (total, g), _ = R.l1_loss(a, b, 0.25)
    assert _same(total, s.detach()) and R.mismatches(g, bd.grad) == 0 and int((g == 0).sum()) >= 205
    assert R.mismatches(R.axpby(0.5, x, -1.25, x)[0], 0.5 * x.double() - 1.25 * x.double()) == 0


@pytest.mark.parametrize('shape', [(3, 16, 32, 32), (2, 100, 96, 32), (1, 64, 64, 1), (1, 64, 64, 64)])
@pytest.mark.parametrize('swish', [False, True])
def test_groupnorm_backward_against_functional(shape, swish):
    n, HW, C, groups = shape
    for zero in (False, True) if shape == R.GN_ZERO else (False,):
        x, da, gamma, beta, _ = R.gn_inputs(n, HW, C, groups, zero)
        xn = x.double().view(n, HW, C).permute(0, 2, 1).clone().requires_grad_(True)
        g, b = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
        t = F.group_norm(xn, groups, g, b, eps=1e-6)
        ((F.silu(t) if swish else t) * da.double().view(n, HW, C).permute(0, 2, 1)).sum().backward()
        (dx, dg, db), (mx, mg, mb) = R.groupnorm_bwd(x, da, gamma, beta, n, HW, C, groups, swish)
        assert torch.isfinite(dx).all() and torch.isfinite(dg).all()
        assert _same(dx, xn.grad.permute(0, 2, 1).reshape(-1, C), 1e-10) and _same(dg, g.grad, 1e-10) and _same(db, b.grad, 1e-10)
        assert bool((mx >= dx.abs() * (1 - 1e-9)).all()) and bool((mg >= dg.abs() * (1 - 1e-9)).all()) and bool((mb >= db.abs() * (1 - 1e-9)).all())


def test_softmax_pose_dense_against_autograd():
    p, dp = R.softmax_inputs(5, 65)
    zz = (torch.log(p.double()) / 0.125).clone().requires_grad_(True)         # p = softmax(scale z) for z = log(p) / scale
    (torch.softmax(zz * 0.125, -1) * dp.double()).sum().backward()
    assert _same(R.softmax_rows_bwd(p, dp, 0.125)[0], zz.grad, 1e-9) and not _same(R.softmax_rows_bwd(p, dp, 1.0)[0], zz.grad, 1e-3)
    rows, L = 257, 64
    raw, gt, wp, wo, div = R.pose_inputs(rows, L)
    (pos, ori, d), (mp, mo, md) = R.pose_mse(raw, gt, wp, wo, div, rows, L, 0.2)
    g = gt.double()[torch.arange(rows) // L]
    pm = float(np.float32(0.2))
    assert _same(pos, F.mse_loss(raw.double()[:, :3] / div.double()[:, None], g[:, :3] * pm, reduction='none').mean(1))
    assert _same(ori, F.mse_loss(raw.double()[:, 3:], g[:, 3:], reduction='none').mean(1))
    assert bool((md >= d.abs() * (1 - 1e-9)).all()) and float(d[0].abs().max()) > 0 and float(d[0, :3].abs().max()) == 0  # w_pos[0] = 0
    rows, K, N = 1000, 7, 129
    x, dy, dW0, db0 = R.dense_inputs(rows, K, N)
    (dW, db), _ = R.dense_small_k_bwd(x, dy, dW0, db0, rows, K, N)
    assert _same(dW, dW0.double() + x.double().t() @ dy.double()) and _same(db, db0.double() + dy.double().sum(0))


def test_lpips_head_against_the_oracle():
    from oracle import lpips_oracle as lo
    n, HW, C = 3, 65, 64
    f0, f1, w, df0 = R.head_inputs(n, HW, C)
    a = f0.double().view(n, HW, C).permute(0, 2, 1).unsqueeze(-1)            # NCHW with W = 1
    b = f1.double().view(n, HW, C).permute(0, 2, 1).unsqueeze(-1).clone().requires_grad_(True)
    d = ((lo.normalize_tensor(a) - lo.normalize_tensor(b)) ** 2 * w.double().view(1, C, 1, 1)).sum((1, 2, 3))
    val, mag = R.lpips_head(f0, f1, w, n, HW, C)
    assert _same(val, d.detach()) and bool((mag >= val.abs()).all())
    (0.37 * d.sum()).backward()
    want = b.grad.squeeze(-1).permute(0, 2, 1).reshape(n * HW, C)
    got, gm = R.lpips_head_bwd(f0, f1, w, df0, n * HW, C, 0.37, False)
    live = f1.double().pow(2).sum(1) > 0
    assert int((~live).sum()) == 2 and not torch.isfinite(want[~live]).all()  # autograd: NaN where |f1| = 0
    assert _same(got[live], want[live], 1e-10) and torch.isfinite(got).all()
    assert float(got[-1].abs().max()) == 0.0 and float(got[0].abs().max()) > 1e6          # f0 = f1 = 0: no gradient; f1 = 0: g / eps
    acc, _ = R.lpips_head_bwd(f0, f1, w, df0, n * HW, C, 0.37, True)
    assert _same(acc, df0.double() + got)


@pytest.mark.parametrize('n', R.CLIP_SIZES[:2])
def test_clip_against_torch(n):
    x = R.clip_input(n)
    norm = float(x.double().norm())
    for max_norm in (0.5 * norm, 2.0 * norm):
        p = torch.nn.Parameter(torch.zeros(n, dtype=F64))
        p.grad = x.double().clone()
        torch.nn.utils.clip_grad_norm_([p], float(np.float32(max_norm)))
        assert _same(R.clip_grad_norm(x, max_norm)[0], p.grad)
        want = x.double() * float(np.float32(max_norm)) / max(norm, float(np.float32(max_norm)))
        assert _same(R.clip_by_norm(x, max_norm)[0], want)
    assert R.mismatches(R.clip_grad_norm(x, 2.0 * norm)[0], x) == 0
    z = torch.zeros(n)
    assert R.mismatches(R.clip_by_norm(z, 1.0)[0], z) == 0 and R.mismatches(R.clip_grad_norm(z, 1.0)[0], z) == 0


def test_scaling_reference():
    x = R.normal((85 * 3,), 8)
    v, m = R.lpips_scaling(x, R.SHIFT3, R.SCALE3, False)
    sh, sc = np.asarray(R.SHIFT3, np.float32).astype(np.float64), np.asarray(R.SCALE3, np.float32).astype(np.float64)
    assert _same(v, torch.from_numpy((x.double().numpy().reshape(-1, 3) - sh) / sc).view(-1))
    xd = x.double().clone().requires_grad_(True)
    (((xd.view(-1, 3) - torch.from_numpy(sh)) / torch.from_numpy(sc)).view(-1) * x.double()).sum().backward()
    assert _same(R.lpips_scaling(x, R.SHIFT3, R.SCALE3, True)[0], xd.grad)


# ------------------------------------------------------------------ 2. the helper rejects what kernels get wrong
C_MUT = 64                      # at least every constant of the GPU test's table


def test_constants_of_the_gpu_test_are_covered():
    import test_hip_training_kernels as G
    assert max(G.C.values()) <= C_MUT


def test_helper_rejects_a_dropped_summand():
    n, HW, C, groups = 2, 100, 96, 32
    x, da, gamma, beta, _ = R.gn_inputs(n, HW, C, groups)
    (dx, dg, db), (mx, mg, mb) = R.groupnorm_bwd(x, da, gamma, beta, n, HW, C, groups, True)
    one = R.groupnorm_bwd(x[:HW], da[:HW], gamma, beta, 1, HW, C, groups, True)[0][1]              # the first image's share only
    assert not R.rejects(dg, dg, mg, C_MUT) and R.rejects(one, dg, mg, C_MUT)
    rows, K, N = 1000, 7, 129
    xs, dy, dW0, db0 = R.dense_inputs(rows, K, N)
    (dW, dbb), (mW, mb2) = R.dense_small_k_bwd(xs, dy, dW0, db0, rows, K, N)
    short = R.dense_small_k_bwd(xs[:-1], dy[:-1], dW0, db0, rows - 1, K, N)[0]
    assert R.rejects(short[0], dW, mW, C_MUT) and R.rejects(short[1], dbb, mb2, C_MUT)
    p, dp = R.softmax_inputs(5, 65)
    v, m = R.softmax_rows_bwd(p, dp, 0.125)
    pm = p.clone()
    pm[:, -1] = 0                                                             # the row sum without its last term
    assert R.rejects(0.125 * p.double() * (dp.double() - (pm.double() * dp.double()).sum(-1, keepdim=True)), v, m, C_MUT)
    f0, f1, w, _ = R.head_inputs(3, 65, 64)
    hv, hm = R.lpips_head(f0, f1, w, 3, 65, 64)
    assert R.rejects(R.lpips_head(f0.view(3, 65, 64)[:, :64].reshape(-1, 64), f1.view(3, 65, 64)[:, :64].reshape(-1, 64), w, 3, 64, 64)[0], hv, hm, C_MUT)
    a, b = R.l1_inputs(2049)
    (s, _), (ms, _) = R.l1_loss(a, b, 1.0)
    assert R.rejects(R.l1_loss(a[:-1], b[:-1], 1.0)[0][0], s, ms, C_MUT)
    xc = R.clip_input(5000)
    cv, cm = R.clip_by_norm(xc, 3.0)
    assert R.rejects(R.t64(xc) * 3.0 / float(R.t64(xc)[:-64].norm()), cv, cm, C_MUT)      # a wave's partial lost from the norm


def test_helper_rejects_a_stale_tail():
    n, Hin, Win, C = 3, 5, 7, 45
    x = R.dyadic((n, Hin, Win, C), 9)
    dst, _ = R.gather_transpose(x, n, Hin, Win, C, Hin, Win, 1, 0, 0)
    for mut in (lambda d: d[-1].zero_(), lambda d: d[:, -1].fill_(-777.0)):   # last channel / last position left stale
        d = dst.clone()
        mut(d)
        assert R.mismatches(d, dst) > 0
    raw, gt, wp, wo, div = R.pose_inputs(257, 64)
    (pos, ori, dr), (mp, mo, md) = R.pose_mse(raw, gt, wp, wo, div, 257, 64, 0.2)
    stale = dr.clone()
    stale[-1] = 0
    assert R.rejects(stale, dr, md, C_MUT)
    wrong_gt = R.pose_mse(raw, gt[torch.arange(257) % gt.shape[0]], wp, wo, div, 257, 1, 0.2)[0][0]      # gt row r instead of r // L
    assert R.rejects(wrong_gt, pos, mp, C_MUT)
    xs = R.normal((85 * 3,), 10)
    v, m = R.lpips_scaling(xs, R.SHIFT3, R.SCALE3, False)
    rolled = R.lpips_scaling(xs, R.SHIFT3[1:] + R.SHIFT3[:1], R.SCALE3[1:] + R.SCALE3[:1], False)[0]       # the channel phase lost on a lap
    assert R.rejects(rolled, v, m, C_MUT)


def test_helper_rejects_a_shifted_window_and_a_second_maximum():
    n, H, W, C = 2, 3, 5, 12
    x = R.dyadic((n, 2 * H, 2 * W, C), 11)
    xv = x.view(n, H, 2, W, 2, C)
    xv[0, 0, :, 0, :, :] = 2.0
    xv[0, 1, 0, 0, :, :] = 8.5                                                # tie (0, 1)
    xv[0, 1, 0, 1, 1, :] = 8.5
    xv[0, 1, 1, 1, 0, :] = 8.5                                                # tie (1, 2)
    xv[0, 2, 1, 2, :, :] = 8.5                                                # tie (2, 3)
    dy = R.dyadic((n, H, W, C), 12, ties=False) + 0.0078125                   # no zero gradient: every misrouting shows
    want, _ = R.maxpool2_bwd(x, dy, n, H, W, C)
    w = R._windows(x, n, H, W, C).numpy()
    last = torch.from_numpy(w.shape[3] - 1 - np.argmax(w[:, :, :, ::-1], axis=3))         # ties sent to the LAST maximum
    dw = torch.zeros((n, H, W, 4, C), dtype=F64).scatter_(3, last.unsqueeze(3), R.t64(dy).view(n, H, W, 1, C))
    bad = torch.zeros((n, H, 2, W, 2, C), dtype=F64)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        bad[:, :, a, :, b] = dw[:, :, :, k]
    assert R.mismatches(bad.reshape(-1, C), want) > 0
    shifted = torch.roll(x.view(n, 2 * H, 2 * W, C), 1, 2)                    # the window one pixel to the left
    assert R.mismatches(R.maxpool2(shifted, n, H, W, C)[0], R.maxpool2(x, n, H, W, C)[0]) > 0
    du = R.dyadic((n, 2 * H, 2 * W, C), 13)
    assert R.mismatches(R.upsample2_bwd(torch.roll(du, 1, 2), n, H, W, C)[0], R.upsample2_bwd(du, n, H, W, C)[0]) > 0
    g0, _ = R.gather_transpose(x, n, 2 * H, 2 * W, C, 2 * H, 2 * W, 1, 0, 0)
    g1, _ = R.gather_transpose(x, n, 2 * H, 2 * W, C, 2 * H, 2 * W, 1, 0, 1)
    assert R.mismatches(g1, g0) > 0


def test_helper_rejects_assignment_for_accumulation():
    n, HW, C, groups = 3, 16, 32, 32
    x, da, gamma, beta, dx0 = R.gn_inputs(n, HW, C, groups)
    (acc, _, _), (macc, _, _) = R.groupnorm_bwd(x, da, gamma, beta, n, HW, C, groups, False, dx0=dx0)
    (plain, _, _), _ = R.groupnorm_bwd(x, da, gamma, beta, n, HW, C, groups, False)
    assert R.rejects(plain, acc, macc, C_MUT) and not R.rejects(acc, acc, macc, C_MUT)
    f0, f1, w, df0 = R.head_inputs(3, 65, 64)
    a, ma = R.lpips_head_bwd(f0, f1, w, df0, 3 * 65, 64, 0.37, True)
    assert R.rejects(R.lpips_head_bwd(f0, f1, w, df0, 3 * 65, 64, 0.37, False)[0], a, ma, C_MUT)
    xs, dy, dW0, db0 = R.dense_inputs(300, 16, 768)
    (dW, db), (mW, mb) = R.dense_small_k_bwd(xs, dy, dW0, db0, 300, 16, 768)
    assert R.rejects(dW - dW0.double(), dW, mW, C_MUT) and R.rejects(db - db0.double(), db, mb, C_MUT)
    assert R.mismatches(R.axpby(1.0, dW0)[0], R.axpby(1.0, dW0, 1.0, dW0)[0]) > 0


def test_helper_treats_nan_and_zero_magnitude_strictly():
    want, mag = torch.tensor([1.0, 0.0]), torch.tensor([1.0, 0.0])
    assert R.rejects(torch.tensor([float('nan'), 0.0]), want, mag, C_MUT)
    assert R.rejects(torch.tensor([1.0, 1e-30]), want, mag, C_MUT) and not R.rejects(torch.tensor([1.0 + 2 ** -24, -0.0]), want, mag, C_MUT)
    assert R.mismatches(torch.tensor([-0.0]), torch.tensor([0.0])) == 0 and R.mismatches(torch.tensor([float('nan')]), torch.tensor([0.0])) == 1


# ------------------------------------------------------------------ 3. calibration
def calibration():
    """kernel -> worst |float32 restatement - float64| / (2^-24 x magnitude) over the GPU test's inputs"""
    out = {}

    def note(k, *triples):
        out[k] = max([out.get(k, 0.0)] + [R.worst_ratio(g, w, m) for g, w, m in triples])
    for npix in R.SCALING_NPIX[:2]:
        x = R.normal((npix * 3,), 20 + npix)
        for bwd in (False, True):
            note('lpips_scaling', (R.lpips_scaling_f32(x, R.SHIFT3, R.SCALE3, bwd),) + R.lpips_scaling(x, R.SHIFT3, R.SCALE3, bwd))
    for (n, HW, C, groups) in R.GN_SHAPES:
        for zero in ((False, True) if (n, HW, C, groups) == R.GN_ZERO else (False,)):
            x, da, gamma, beta, dx0 = R.gn_inputs(n, HW, C, groups, zero)
            mean_c, scale_c, rstd = R.gn_stats_f32(x, gamma, n, HW, C, groups)
            for swish in (False, True):
                for d0 in (None, dx0):
                    got = R.groupnorm_bwd_f32(x, da, mean_c, scale_c, rstd, gamma, beta, n, HW, C, groups, swish, d0)
                    want, mag = R.groupnorm_bwd(x, da, gamma, beta, n, HW, C, groups, swish, dx0=d0)
                    note('groupnorm_bwd', *zip(got, want, mag))
    for rows, n in R.SOFTMAX_CASES:
        p, dp = R.softmax_inputs(rows, n)
        for scale in (1.0, 0.125):
            note('softmax_rows_bwd_', (R.softmax_rows_bwd_f32(p, dp, scale),) + R.softmax_rows_bwd(p, dp, scale))
    for n, HW, C in R.HEAD_CASES:
        f0, f1, w, df0 = R.head_inputs(n, HW, C)
        note('lpips_head', (R.lpips_head_f32(f0, f1, w, n, HW, C),) + R.lpips_head(f0, f1, w, n, HW, C))
        for acc in (False, True):
            note('lpips_head_bwd', (R.lpips_head_bwd_f32(f0, f1, w, df0, n * HW, C, 0.37, acc),) + R.lpips_head_bwd(f0, f1, w, df0, n * HW, C, 0.37, acc))
    for rows, L in R.POSE_CASES:
        raw, gt, wp, wo, div = R.pose_inputs(rows, L)
        for dv in (None, div):
            want, mag = R.pose_mse(raw, gt, wp, wo, dv, rows, L, 0.2)
            note('pose_mse', *zip(R.pose_mse_f32(raw, gt, wp, wo, dv, rows, L, 0.2), want, mag))
    for rows, K, N in R.DENSE_CASES:
        x, dy, dW0, db0 = R.dense_inputs(rows, K, N)
        want, mag = R.dense_small_k_bwd(x, dy, dW0, db0, rows, K, N)
        note('dense_small_k_bwd', *zip(R.dense_small_k_bwd_f32(x, dy, dW0, db0, rows, K, N), want, mag))
    for n in R.CLIP_SIZES:
        x = R.clip_input(n)
        norm = float(x.double().norm())
        for lim in (0.5 * norm, 2.0 * norm):
            note('clip_by_norm_', (R.clip_by_norm_f32(x, lim),) + R.clip_by_norm(x, lim))
            note('clip_grad_norm_', (R.clip_grad_norm_f32(x, lim),) + R.clip_grad_norm(x, lim))
    for n in R.L1_SIZES:
        a, b = R.l1_inputs(n)
        (s, _), (m, _) = R.l1_loss(a, b, 1.0)
        note('l1_loss', (R.l1_sum_f32(a, b), s, m))
    return out


def _pow2_ceil(v):
    return 2.0 ** int(np.ceil(np.log2(max(v, 2.0 ** -20))))


def test_calibration_covers_the_gpu_tests_constants():
    """c = 4 x the float32 CPU restatement's worst error, rounded up to a power of two (GroupNorm backward: 32, the basis measured when the
    test was specified; this run's own basis must not exceed it).  The restatement's own sums depend on how torch splits them, so the
    table may sit one binade from this run's figure, never further"""
    import test_hip_training_kernels as G
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        cal = calibration()
    finally:
        torch.set_num_threads(threads)
    for k in sorted(cal):
        print(f'calibration {k}: fp32 CPU restatement worst {cal[k]:.2f} units of 2^-24 x magnitude -> c = {_pow2_ceil(4 * cal[k]):g} (table: {G.C[k]:g})')
    assert set(cal) == set(G.C)
    for k, v in cal.items():
        assert _pow2_ceil(4 * v) <= 2 * G.C[k] and G.C[k] <= (32.0 if k == 'groupnorm_bwd' else 2 * _pow2_ceil(4 * v)), (k, v, G.C[k])
