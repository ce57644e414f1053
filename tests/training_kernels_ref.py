"""Test infrastructure of the per-kernel tests of the codebook trainer, the LPIPS loss and the transformer trainer's loss / clip path
(tests/test_hip_training_kernels.py on the GPU, tests/test_training_kernels_ref_host.py on the CPU).

For every kernel: a float64 restatement written from the operation's definition in the kernel's own layout (NHWC rows, [C][P] for the
gather, [K][N] for dW), autograd where the operation has a gradient.  A reference returns ``(value, magnitude)``: the magnitude is the
same expression with every summand replaced by its absolute value — the scale rounding is judged against — and None where the kernel
is in the exact class (copies, selections, sums of at most four terms of dyadic inputs).  ``*_f32`` functions restate the KERNEL's
formula on plain torch-CPU float32 ops: the host test measures their distance from fp64 (in units of 2^-24 x magnitude) on the very
inputs of the GPU test, and the GPU test's constants come from that measurement, never from the kernel.  The input generators and the
case lists live here so that both files see the same tensors."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                  # unit roundoff of float32
F64 = torch.float64


def t64(a):
    """float64 on the tensor's own device (the largest cases hand over device tensors: the same torch float64 statement runs there)"""
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(F64)


# ------------------------------------------------------------------ inputs
def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def dyadic(shape, seed, ties=True):
    """float32 multiples of 2^-6 in [-8, 8] with exact zeros, -0.0 and (``ties``) runs of repeated values: every fp32 sum of four such
    numbers and every product with a multiple of 2^-3 below 8 is exact"""
    g = rng(seed)
    a = (g.integers(-512, 513, size=shape).astype(np.float32) / 64.0).reshape(-1)
    n = a.size
    k = max(1, n // 16)
    a[g.integers(0, n, size=k)] = 0.0
    a[g.integers(0, n, size=k)] = -0.0
    if ties and n >= 8:
        i = g.integers(0, n - 1, size=max(1, n // 8))
        a[i + 1] = a[i]
    return torch.from_numpy(a.reshape(shape))


def normal(shape, seed, std=1.0, mean=0.0):
    return torch.from_numpy((rng(seed).standard_normal(size=shape) * std + mean).astype(np.float32))


# ------------------------------------------------------------------ the comparison helper
def mismatches(got, want):
    """exact class: number of elements whose VALUES differ (-0 == +0; a NaN differs from everything)"""
    got, want = t64(got), t64(want)
    if got.shape != want.shape:
        return max(got.numel(), want.numel(), 1)
    return int((~(got == want)).sum())


def worst_ratio(got, want, mag):
    """rounded class: max over elements of |got - want| / (2^-24 x magnitude); an element of zero magnitude must be matched exactly and a
    non-finite result counts as infinitely far"""
    got, want, mag = t64(got), t64(want), t64(mag)
    if got.shape != want.shape:
        return float('inf')
    if got.numel() == 0:
        return 0.0
    err = (got - want).abs()
    r = torch.where(mag > 0, err / (U * mag.clamp_min(1e-300)), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))
    return float(r.max())


def rejects(got, want, mag, c):
    return not worst_ratio(got, want, mag) <= c


# ------------------------------------------------------------------ exact class
def gather_transpose(src, n, Hin, Win, C, Hout, Wout, stride, oy, ox):
    """dst[c][(img, y, x)] = src[img][y*stride + oy][x*stride + ox][c], zero outside the image"""
    s = t64(src).view(n, Hin, Win, C)
    dst = torch.zeros((C, n, Hout, Wout), dtype=F64)
    for y in range(Hout):
        sy = y * stride + oy
        if not 0 <= sy < Hin:
            continue
        for x in range(Wout):
            sx = x * stride + ox
            if 0 <= sx < Win:
                dst[:, :, y, x] = s[:, sy, sx, :].t()
    return dst.view(C, n * Hout * Wout), None


def upsample2_bwd(du, n, H, W, C):
    """gradient of the nearest x2 upsample: the sum of each 2x2 block of du [n][2H][2W][C]"""
    d = t64(du).view(n, H, 2, W, 2, C)
    return ((d[:, :, 0, :, 0] + d[:, :, 0, :, 1]) + d[:, :, 1, :, 0] + d[:, :, 1, :, 1]).reshape(n * H * W, C), None


def relu(x):
    x = t64(x)
    return torch.where(x > 0, x, torch.zeros_like(x)), None


def relu_bwd(dy, y):
    dy, y = t64(dy), t64(y)
    return torch.where(y > 0, dy, torch.zeros_like(dy)), None


def _windows(x, n, Hout, Wout, C):
    """[n][Hout][Wout][4][C]: the 2x2 window of every output in row-major order"""
    v = t64(x).view(n, Hout, 2, Wout, 2, C)
    return torch.stack((v[:, :, 0, :, 0], v[:, :, 0, :, 1], v[:, :, 1, :, 0], v[:, :, 1, :, 1]), 3)


def maxpool2(x, n, Hout, Wout, C):
    return _windows(x, n, Hout, Wout, C).max(3).values.reshape(n * Hout * Wout, C), None


def maxpool2_bwd(x, dy, n, Hout, Wout, C):
    """the gradient of an output goes to the FIRST maximum of its window in row-major order"""
    w = _windows(x, n, Hout, Wout, C)
    pos = torch.arange(4, device=w.device).view(1, 1, 1, 4, 1)
    first = torch.where(w == w.max(3, keepdim=True).values, pos, 4).min(3).values     # the smallest position that holds the maximum
    g = t64(dy).view(n, Hout, Wout, C)
    dw = torch.zeros_like(w)
    dw.scatter_(3, first.unsqueeze(3), g.unsqueeze(3))
    dx = torch.zeros((n, Hout, 2, Wout, 2, C), dtype=F64, device=w.device)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, :, a, :, b] = dw[:, :, :, k]
    return dx.reshape(n * Hout * 2 * Wout * 2, C), None


def axpby(a, x, b=0.0, y=None):
    v = float(a) * t64(x)
    return (v + float(b) * t64(y) if y is not None else v), None


def l1_loss(x, y, w):
    """-> ((sum |y - x|, dy = sign(y - x) w), (the same sum: all its terms are positive, None: dy is exact))"""
    d = t64(y) - t64(x)
    s = d.abs().sum()
    return (s, torch.sign(d) * float(np.float32(w))), (s, None)


# ------------------------------------------------------------------ rounded class
def lpips_scaling(x, shift3, scale3, backward):
    """rows of 3 channels: (x - shift) / scale, backward x / scale; shift / scale as the float32 values the entry point receives"""
    x = t64(x).view(-1, 3)
    sh = t64(np.asarray(shift3, np.float32)).to(x.device)
    sc = t64(np.asarray(scale3, np.float32)).to(x.device)
    if backward:
        return (x / sc).view(-1), (x.abs() / sc.abs()).view(-1)
    return ((x - sh) / sc).view(-1), ((x.abs() + sh.abs()) / sc.abs()).view(-1)


def lpips_scaling_f32(x, shift3, scale3, backward):
    x = x.float().view(-1, 3)
    sh, sc = torch.tensor(shift3, dtype=torch.float32), torch.tensor(scale3, dtype=torch.float32)
    return (x / sc if backward else (x - sh) / sc).view(-1)


def _swish_grad_abs(t, t_abs):
    s = torch.sigmoid(t)
    return s * (1 + t_abs * (1 - s))


def groupnorm_stats(x, n, HW, C, groups, eps):
    """-> (mean, rstd) [n][groups] of the biased variance, as torch.nn.GroupNorm"""
    v = t64(x).view(n, HW, groups, C // groups)
    mean = v.mean((1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean((1, 3))
    return mean, 1.0 / torch.sqrt(var + eps)


def groupnorm_bwd(x, da, gamma, beta, n, HW, C, groups, swish, eps=1e-6, dx0=None):
    """a = swish?(xhat gamma + beta), xhat = (x - mean) rstd per (image, group) -> gradients of sum(a da) by autograd:
    ((dx [+ dx0], dgamma, dbeta), magnitudes).  Magnitudes: xhat -> (|x| + |mean|) rstd, t -> |xhat| |gamma| + |beta|, the swish
    derivative s (1 + t (1 - s)) with |t|, dx = rstd (gamma dt - mean(gamma dt) - xhat mean(gamma dt xhat)) term by term."""
    cg = C // groups
    xv = t64(x).view(n, HW, groups, cg).clone().requires_grad_(True)
    g = t64(gamma).view(groups, cg).clone().requires_grad_(True)
    b = t64(beta).view(groups, cg).clone().requires_grad_(True)
    dav = t64(da).view(n, HW, groups, cg)
    mean = xv.mean((1, 3), keepdim=True)
    var = ((xv - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    t = (xv - mean) * rstd * g + b
    a = t * torch.sigmoid(t) if swish else t
    (a * dav).sum().backward()
    dx = xv.grad.reshape(n * HW, C)
    if dx0 is not None:
        dx = dx + t64(dx0).view(n * HW, C)
    with torch.no_grad():
        xh_a = (xv.abs() + mean.abs()) * rstd
        dt_a = dav.abs() * (_swish_grad_abs(t, xh_a * g.abs() + b.abs()) if swish else 1.0)
        m1 = (g.abs() * dt_a).mean((1, 3), keepdim=True)
        m2 = (g.abs() * dt_a * xh_a).mean((1, 3), keepdim=True)
        mdx = (rstd * (g.abs() * dt_a + m1 + xh_a * m2)).reshape(n * HW, C)
        if dx0 is not None:
            mdx = mdx + t64(dx0).view(n * HW, C).abs()
        mg = (dt_a * xh_a).sum((0, 1)).reshape(C)
        mb = dt_a.sum((0, 1)).reshape(C)
    return (dx.detach(), g.grad.reshape(C), b.grad.reshape(C)), (mdx, mg, mb)


def groupnorm_bwd_f32(x, da, mean_c, scale_c, rstd_g, gamma, beta, n, HW, C, groups, swish, dx0=None):
    """the kernel's formula on float32: per-channel mean / scale = rstd gamma [n][C] and the per-(image, group) rstd [n][groups]"""
    cg = C // groups
    xc = x.float().view(n, HW, C) - mean_c.float().view(n, 1, C)
    dt = da.float().view(n, HW, C).clone()
    if swish:
        t = xc * scale_c.float().view(n, 1, C) + beta.float()
        s = 1.0 / (1.0 + torch.exp(-t))
        dt = dt * (s * (1.0 + t * (1.0 - s)))
    rs = rstd_g.float().repeat_interleave(cg, 1).view(n, 1, C)
    s1, s2 = dt.sum(1), (dt * xc).sum(1)                                                 # [n][C]
    inv = 1.0 / (HW * cg)
    m1 = ((gamma.float() * s1).view(n, groups, cg).sum(2) * inv).repeat_interleave(cg, 1).view(n, 1, C)
    m2 = ((gamma.float() * s2).view(n, groups, cg).sum(2) * inv).repeat_interleave(cg, 1).view(n, 1, C) * rs
    dx = rs * (gamma.float() * dt - m1 - (xc * rs) * m2)
    if dx0 is not None:
        dx = dx0.float().view(n, HW, C) + dx
    return dx.reshape(n * HW, C), (rs.view(n, C) * s2).sum(0), s1.sum(0)


def softmax_rows_bwd(p, dp, scale):
    """ds = scale p (dp - sum_j p_j dp_j)"""
    p, dp = t64(p), t64(dp)
    s = (p * dp).sum(-1, keepdim=True)
    sa = (p * dp.abs()).sum(-1, keepdim=True)
    return scale * p * (dp - s), abs(scale) * p * (dp.abs() + sa)


def softmax_rows_bwd_f32(p, dp, scale):
    p, dp = p.float(), dp.float()
    return torch.tensor(scale, dtype=torch.float32) * p * (dp - (p * dp).sum(-1, keepdim=True))


LPIPS_EPS = 1e-10


def lpips_head(f0, f1, w, n, HW, C):
    """per image: sum over pixels of sum_c w_c (f0_c / (|f0| + eps) - f1_c / (|f1| + eps))^2"""
    a, b, w = t64(f0).view(n, HW, C), t64(f1).view(n, HW, C), t64(w)
    na = a.pow(2).sum(-1, keepdim=True).sqrt() + LPIPS_EPS
    nb = b.pow(2).sum(-1, keepdim=True).sqrt() + LPIPS_EPS
    return (w * (a / na - b / nb) ** 2).sum((1, 2)), (w.abs() * (a.abs() / na + b.abs() / nb) ** 2).sum((1, 2))


def lpips_head_f32(f0, f1, w, n, HW, C):
    a, b, w = f0.float().view(n, HW, C), f1.float().view(n, HW, C), w.float()
    na = a.pow(2).sum(-1, keepdim=True).sqrt() + torch.tensor(1e-10, dtype=torch.float32)
    nb = b.pow(2).sum(-1, keepdim=True).sqrt() + torch.tensor(1e-10, dtype=torch.float32)
    return (w * (a / na - b / nb) ** 2).sum((1, 2))


def _lpips_head_bwd(a, b, w, gscale, df0, accumulate, eps, absolute):
    na = a.pow(2).sum(-1, keepdim=True).sqrt() + eps
    s = b.pow(2).sum(-1, keepdim=True).sqrt()
    nb = s + eps
    if absolute:
        g = 2 * w.abs() * (a.abs() / na + b.abs() / nb)
        dot = (g * b.abs()).sum(-1, keepdim=True)
    else:
        g = -2 * w * (a / na - b / nb)
        dot = (g * b).sum(-1, keepdim=True)
    # d|b| / db is undefined at b = 0 (autograd: NaN); the convention there, stated by the kernel as well, is k = 0
    k = torch.where(s > 0, dot / (nb * nb * torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(dot))
    if absolute:
        v = abs(gscale) * (g / nb + k * b.abs())
        return df0.abs() + v if accumulate else v
    v = gscale * (g / nb - k * b)
    return df0 + v if accumulate else v


def lpips_head_bwd(f0, f1, w, df1, npix, C, gscale, accumulate):
    """df1 (+)= gscale d/df1 of the head: with bhat = b / nb, nb = |b| + eps, g = -2 w (ahat - bhat):
    d/db_j = g_j / nb - (sum_c g_c b_c) b_j / (nb^2 |b|), and k = 0 where |b| = 0"""
    a, b, w, d0 = t64(f0).view(npix, C), t64(f1).view(npix, C), t64(w), t64(df1).view(npix, C)
    return (_lpips_head_bwd(a, b, w, gscale, d0, accumulate, LPIPS_EPS, False),
            _lpips_head_bwd(a, b, w, gscale, d0, accumulate, LPIPS_EPS, True))


def lpips_head_bwd_f32(f0, f1, w, df1, npix, C, gscale, accumulate):
    a, b, w, d0 = f0.float().view(npix, C), f1.float().view(npix, C), w.float(), df1.float().view(npix, C)
    return _lpips_head_bwd(a, b, w, torch.tensor(gscale, dtype=torch.float32), d0, accumulate, torch.tensor(1e-10, dtype=torch.float32), False)


def pose_mse(raw, gt, w_pos, w_ori, xyz_div, rows, L, pm):
    """per row r (gt row r // L): pos = mean_3 (raw / div - gt pm)^2, ori = mean_4 (raw - gt)^2, draw by autograd of
    sum(w_pos pos + w_ori ori) -> ((pos, ori, draw), magnitudes)"""
    x = t64(raw).view(rows, 7).clone().requires_grad_(True)
    g = t64(gt).view(-1, 7)[torch.arange(rows) // L]
    wp, wo = t64(w_pos), t64(w_ori)
    dv = t64(xyz_div).view(rows, 1) if xyz_div is not None else torch.ones((rows, 1), dtype=F64)
    pmf = float(np.float32(pm))
    ep, eo = x[:, :3] / dv - g[:, :3] * pmf, x[:, 3:] - g[:, 3:]
    pos, ori = (ep ** 2).mean(1), (eo ** 2).mean(1)
    (wp * pos + wo * ori).sum().backward()
    with torch.no_grad():
        ap = x[:, :3].abs() / dv.abs() + (g[:, :3] * pmf).abs()
        ao = x[:, 3:].abs() + g[:, 3:].abs()
        md = torch.cat((2 * ap / 3 * (wp.abs().view(-1, 1) / dv.abs()), 2 * ao / 4 * wo.abs().view(-1, 1)), 1)
    return (pos.detach(), ori.detach(), x.grad), ((ap ** 2).mean(1), (ao ** 2).mean(1), md)


def pose_mse_f32(raw, gt, w_pos, w_ori, xyz_div, rows, L, pm):
    x = raw.float().view(rows, 7)
    g = gt.float().view(-1, 7)[torch.arange(rows) // L]
    dv = xyz_div.float().view(rows, 1) if xyz_div is not None else torch.ones((rows, 1))
    ep, eo = x[:, :3] / dv - g[:, :3] * torch.tensor(pm, dtype=torch.float32), x[:, 3:] - g[:, 3:]
    d = torch.cat((2.0 * ep / 3.0 * w_pos.float().view(-1, 1) / dv, 2.0 * eo / 4.0 * w_ori.float().view(-1, 1)), 1)
    return (ep * ep).sum(1) / 3.0, (eo * eo).sum(1) / 4.0, d


def dense_small_k_bwd(x, dy, dW0, db0, rows, K, N):
    """dW [K][N] += x^T dy, db += column sums of dy (autograd of y = x W + b)"""
    xv, dyv = t64(x).view(rows, K), t64(dy).view(rows, N)
    W = torch.zeros((K, N), dtype=F64, requires_grad=True)
    b = torch.zeros(N, dtype=F64, requires_grad=True)
    ((xv @ W + b) * dyv).sum().backward()
    return ((t64(dW0) + W.grad, t64(db0) + b.grad),
            (t64(dW0).abs() + xv.abs().t() @ dyv.abs(), t64(db0).abs() + dyv.abs().sum(0)))


def dense_small_k_bwd_f32(x, dy, dW0, db0, rows, K, N):
    return dW0.float() + x.float().view(rows, K).t() @ dy.float().view(rows, N), db0.float() + dy.float().view(rows, N).sum(0)


def clip_by_norm(x, clip):
    """tf.clip_by_norm: x clip / max(||x||, clip)"""
    x = t64(x)
    v = x * (float(np.float32(clip)) / max(float(x.norm()), float(np.float32(clip))))
    return v, v.abs()


def clip_grad_norm(x, max_norm):
    """torch.nn.utils.clip_grad_norm_: x max_norm / (||x|| + 1e-6), applied only when that factor is below 1"""
    x = t64(x)
    f = float(np.float32(max_norm)) / (float(x.norm()) + 1e-6)
    v = x * f if f < 1.0 else x.clone()
    return v, v.abs()


def clip_by_norm_f32(x, clip):
    x = x.float()
    c = torch.tensor(clip, dtype=torch.float32)
    return x * (c / torch.maximum((x * x).sum().sqrt(), c))


def clip_grad_norm_f32(x, max_norm):
    x = x.float()
    f = torch.tensor(max_norm, dtype=torch.float32) / ((x * x).sum().sqrt() + torch.tensor(1e-6, dtype=torch.float32))
    return x * f if bool(f < 1.0) else x.clone()


def l1_sum_f32(x, y):
    return (y.float() - x.float()).abs().sum()


# ------------------------------------------------------------------ the cases of the rounded class (shared by the CPU calibration and the GPU test)
SHIFT3, SCALE3 = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)                 # lpips ScalingLayer

GN_SHAPES = [(3, 16, 32, 32), (2, 100, 96, 32), (1, 130, 320, 32), (1, 4160, 64, 32), (2, 64, 1024, 32), (1, 64, 64, 1), (1, 64, 64, 64)]
GN_ZERO = (2, 100, 96, 32)


def gn_inputs(n, HW, C, groups, zero_gains=False):
    """x with a non-zero mean, beta != 0; ``zero_gains``: gamma[1] = 0, gamma[C-2] = 1e-30 and the whole of group 2 zero"""
    seed = 1000 + 7 * HW + C + groups
    x, da = normal((n * HW, C), seed, 2.0, 0.5), normal((n * HW, C), seed + 1)
    gamma, beta = normal((C,), seed + 2, 0.3, 1.0), normal((C,), seed + 3, 0.2, 0.1)
    dx0 = normal((n * HW, C), seed + 4)
    if zero_gains:
        cg = C // groups
        gamma[1] = 0.0
        gamma[C - 2] = 1e-30
        gamma[2 * cg:3 * cg] = 0.0
    return x, da, gamma, beta, dx0


def gn_stats_f32(x, gamma, n, HW, C, groups, eps=1e-6):
    """float32 (mean_c, scale_c = rstd gamma) [n][C] and rstd [n][groups] rounded from the float64 statistics: what the forward hands to
    the backward (the GPU test takes them from ops.groupnorm_stats wherever that entry point accepts the channel count)"""
    mean, rstd = groupnorm_stats(x, n, HW, C, groups, eps)
    cg = C // groups
    mean32, rstd32 = mean.float(), rstd.float()
    return mean32.repeat_interleave(cg, 1).contiguous(), (rstd32.repeat_interleave(cg, 1) * gamma.float()).contiguous(), rstd32


SOFTMAX_CASES = [(rows, n) for rows in (1, 5, 1027) for n in (1, 63, 64, 65, 1000)]


def softmax_inputs(rows, n):
    logits = normal((rows, n), 50 + rows + n, 2.0).double()
    logits[rows // 2, n // 3] += 40.0                                            # one row nearly one-hot
    return torch.softmax(logits, -1).float(), normal((rows, n), 51 + rows + n)


HEAD_CASES = [(n, HW, C) for n in (1, 3) for HW in (1, 63, 64, 65, 100) for C in (64, 96, 512)]
HEAD_BIG = (1, 4 * 65536 + 7, 64)                                               # the backward's grid-stride loop takes a second lap


def head_inputs(n, HW, C, seed=0):
    """features after a ReLU (zeros are common); pixel 0 has f1 == 0 where there is more than one pixel, the last pixel f0 == f1 == 0"""
    f0 = normal((n * HW, C), 70 + HW + C + seed).clamp_min(0)
    f1 = (f0 + normal((n * HW, C), 71 + HW + C + seed, 0.3)).clamp_min(0)
    w = normal((C,), 72 + C, 0.5)
    if n * HW > 1:
        f1[0] = 0.0
        f0[-1] = 0.0
        f1[-1] = 0.0
    else:
        f1[0] = 0.0
    return f0, f1, w, normal((n * HW, C), 73 + HW + C)


POSE_CASES = [(rows, L) for L in (1, 64) for rows in (1, 255, 256, 257)]


def pose_inputs(rows, L):
    nb = (rows + L - 1) // L
    raw, gt = normal((rows, 7), 90 + rows + L), normal((nb, 7), 91 + rows + L)
    wp, wo = torch.from_numpy(rng(92 + rows).uniform(0, 1, rows).astype(np.float32)), torch.from_numpy(rng(93 + rows).uniform(0, 1, rows).astype(np.float32))
    wp[::3] = 0.0
    wo[1::4] = 0.0
    div = torch.from_numpy(rng(94 + rows).uniform(0.5, 2.0, rows).astype(np.float32))
    return raw, gt, wp, wo, div


DENSE_CASES = [(1, 1, 1), (1000, 7, 129), (300, 16, 768)]


def dense_inputs(rows, K, N):
    return normal((rows, K), 110 + K), normal((rows, N), 111 + N), normal((K, N), 112 + K), normal((N,), 113 + N)


CLIP_SIZES = [1, 5000, 3 * 2 ** 20 + 3]


def clip_input(n):
    return normal((n,), 130 + n % 97)


L1_SIZES = [1, 2047, 2048, 2049, 1024 * 2048 + 1]


def l1_inputs(n):
    x, y = normal((n,), 150 + n % 89), normal((n,), 151 + n % 89)
    y[::10] = x[::10]                                                            # a tenth equal: dy = 0 there
    return x, y


SCALING_NPIX = [1, 85, 16384 * 256 // 3 + 7]
