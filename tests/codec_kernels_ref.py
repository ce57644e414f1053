"""Test infrastructure of the per-kernel tests of the image codec's glue kernels (tests/test_hip_codec_kernels.py on the GPU,
tests/test_codec_kernels_ref_host.py on the CPU): GroupNorm statistics / finalize / apply, the GroupNorm prologue of the 1x1 GEMMs, the
AttnBlock's spatial attention, the codebook kernels, conv_in and the convolution to a handful of channels.  Host only: plain torch /
numpy float64, nothing here touches the GPU or imports viewformer_amd.

For every kernel: a float64 reference written from the operation's definition in the kernel's own layout, returning the value and the
MAGNITUDE rounding is judged against (the same expression with every summand replaced by its absolute value); the input generators
and case tables both test files share; and ``*_f32`` functions that restate the KERNEL's summation order on the CPU in float32
(sequential chains where the kernel runs one).  The restatements exist for calibration only: the host file measures their distance
from float64 in units of 2^-24 x magnitude on the very inputs of the GPU test, and every constant ``c`` of the GPU test is 4 x that
figure rounded up to a power of two, never a figure of the kernel.  ``defect=...`` evaluates a reference with one deliberate mistake
(the discrimination controls of the host file)."""
import numpy as np
import torch
import torch.nn.functional as F

import conv_kernels_ref as CR
import training_kernels_ref as T

U = T.U
F64 = torch.float64
t64, rng, normal, mismatches, worst_ratio = T.t64, T.rng, T.normal, T.mismatches, T.worst_ratio
EPS = float(np.float32(1e-6))                        # the eps every caller hands over, as the float the kernels receive

# standing rules, quoted (never relaxed here)
X6_MAX, X6_RMS = CR.X6_MAX, CR.X6_RMS                # tests/test_hip_x6.py, test_hip_x3h.py: max error < 6e-7 of magnitude, rms < 1.25 x native f32 + 1e-9
CONV_IN_X3H_MAX = 4e-7                               # tests/test_hip_x3h.py::test_conv_in_x3h_matches_fp64_and_the_valu_kernel
GN_MEAN_TOL, GN_SCALE_TOL = CR.GN_MEAN_TOL, CR.GN_SCALE_TOL      # fused statistics (tests/test_hip_conv_kernels.py)
ATTN_X3H_MUL, ATTN_X3H_ABS = 1.25, 2e-7              # tests/test_hip_models.py: e3h < 1.25 e32 + 2e-7 max(1, max |ref|)
# vf_common.h: vf_swish = "precise expf + IEEE division": expf to 1 ulp (2 units of 2^-24, weighted by e / (1 + e) <= 1), one rounding of
# 1 + e and one of the division: 4 units of 2^-24 x |swish(t)|.  vf_swish_1ulp = "x * sigmoid(x) to ~1.5 ulp": 3 units.
SWISH_U, SWISH_1ULP_U = 4.0, 3.0
SWISH_LIP = 1.1                                      # max |swish'(t)| = 1.0998: what an error of t becomes behind the swish


def pow2_ceil(v):
    return 2.0 ** int(np.ceil(np.log2(max(v, 2.0 ** -20))))


def seq_matmul_f32(a, b):
    """a [..., M, K] @ b [..., K, N] in float32 as ONE ascending chain over k per output (the f32 MFMA / fmaf chains of the kernels),
    product and sum rounded separately"""
    a, b = a.float(), b.float()
    acc = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=torch.float32)
    for k in range(a.shape[-1]):
        acc = acc + a[..., :, k, None] * b[..., k, None, :]
    return acc


def swish(t):
    return t * torch.sigmoid(t)


def swish_f32(t):
    t = t.float()
    return t / (1.0 + torch.exp(-t))


# ================================================================== GroupNorm statistics
# (C, groups, HW), n = 3 throughout
STATS_N = 3
STATS_ROWS = [(4, 1, 300), (4, 4, 7), (32, 32, 1), (128, 32, 255), (128, 32, 513), (256, 32, 1000), (512, 32, 64), (1024, 32, 257),
              (1024, 256, 64), (128, 8, 16385)]
STATS_RATIOS = (0.0, 0.5, 10.0, 30.0, 100.0)         # mean / std of the calibration classes
STATS_CLASSES = ('n15', 'groups') + STATS_RATIOS     # N(1.5, 3) as test_hip_ops.py; per-group offset and scale over three decades
STATS_REFUSED = [(96, 32), (2048, 32), (6, 1), (1024, 512), (128, 48)]        # (C, groups): all UNSUPPORTED


def stats_seed(row, cls):
    C, groups, HW = row
    return 100003 + 31 * C + 17 * groups + 13 * HW + 7 * STATS_CLASSES.index(cls)


def stats_inputs(row, cls):
    """-> x rows [n HW][C], gamma [C] (gamma[0] = 0, gamma[C - 1] < 0)"""
    C, groups, HW = row
    n, s = STATS_N, stats_seed(row, cls)
    if cls == 'n15':
        x = normal((n * HW, C), s, 3.0, 1.5)
    elif cls == 'groups':
        g = rng(s + 1)
        scale = 10.0 ** (g.permutation(groups) / max(groups - 1, 1) * 3.0 - 1.5)                     # 10^-1.5 .. 10^1.5, one per group
        off = scale * g.uniform(1.0, 3.0, size=groups) * g.choice([-1.0, 1.0], size=groups)
        cg = C // groups
        x = normal((n * HW, C), s) * torch.from_numpy(np.repeat(scale, cg).astype(np.float32)) + torch.from_numpy(np.repeat(off, cg).astype(np.float32))
    else:
        x = normal((n * HW, C), s, 1.0, float(cls))
    gamma = normal((C,), s + 2, 0.3, 1.0)
    gamma[0] = 0.0
    gamma[C - 1] = -0.75
    return x, gamma


def gn_ref(x_rows, n, HW, C, groups, eps=EPS, defect=None):
    """float64 (mean, var, rstd) [n][groups] of rows [n HW][C].  Defects: 'drop_last' = the last pixel of every split of the statistics
    kernel is not summed (but counted); 'unbiased' = the variance divided by N - 1; 'no_eps'"""
    cg = C // groups
    xg = t64(x_rows).view(n, HW, groups, cg)
    N = HW * cg
    if defect == 'drop_last':
        keep = torch.ones(HW, dtype=F64)
        ns = gn_nsplit(HW)
        per = (HW + ns - 1) // ns
        for s in range(ns):
            keep[min(HW, s * per + per) - 1] = 0.0
        xg = xg * keep.view(1, HW, 1, 1)
    mean = xg.sum(dim=(1, 3)) / N
    var = (xg * xg).sum(dim=(1, 3)) / N - mean * mean
    if defect != 'drop_last':                        # (the centred form where nothing was dropped: no cancellation in the reference)
        var = ((xg - mean.view(n, 1, groups, 1)) ** 2).sum(dim=(1, 3)) / N
    if defect == 'unbiased':
        var = var * N / max(N - 1, 1)
    rstd = 1.0 / torch.sqrt(var.clamp_min(0) + (0.0 if defect == 'no_eps' else eps))
    return mean, var, rstd


def gn_channels(mean, rstd, gamma, C):
    """(mean_c, scale_c) [n][C] float64 as the kernels lay them out"""
    cg = C // mean.shape[1]
    return mean.repeat_interleave(cg, 1), rstd.repeat_interleave(cg, 1) * t64(gamma)


def gn_nsplit(HW):
    return max(1, min(64, HW // 256))


def gn_partials_f32(x_rows, n, HW, C, groups):
    """the statistics kernel's fp32 partials [n][nsplit][groups][2] in its summation order: per split, 256 / (C / 4) pixel lanes each
    striding over the split's pixels, then the lanes in order per channel, then the group's channels in order"""
    x = x_rows.float().view(n, HW, C)
    ns = gn_nsplit(HW)
    per = (HW + ns - 1) // ns
    ppp = 256 // (C // 4)
    cg = C // groups
    out = torch.zeros((n, ns, groups, 2), dtype=torch.float32)
    for s in range(ns):
        xs = x[:, s * per:min(HW, s * per + per)]
        it = (xs.shape[1] + ppp - 1) // ppp
        xs = F.pad(xs, (0, 0, 0, it * ppp - xs.shape[1])).view(n, it, ppp, C)      # (a lane past the end adds nothing)
        a = torch.zeros((n, ppp, C), dtype=torch.float32)
        b = torch.zeros((n, ppp, C), dtype=torch.float32)
        for i in range(it):
            a = a + xs[:, i]
            b = b + xs[:, i] * xs[:, i]
        ca, cb = torch.zeros((n, C), dtype=torch.float32), torch.zeros((n, C), dtype=torch.float32)
        for k in range(ppp):
            ca, cb = ca + a[:, k], cb + b[:, k]
        ca, cb = ca.view(n, groups, cg), cb.view(n, groups, cg)
        ga, gb = torch.zeros((n, groups), dtype=torch.float32), torch.zeros((n, groups), dtype=torch.float32)
        for k in range(cg):
            ga, gb = ga + ca[:, :, k], gb + cb[:, :, k]
        out[:, s, :, 0], out[:, s, :, 1] = ga, gb
    return out


def finalize_ref(part, HW, cg, eps=EPS, defect=None):
    """float64 (mean, var (unclamped), rstd) [n][groups] of fp32 partials [n][nslots][groups][2], summed in float64.
    Defect 'drop_slot': the last slot is not added"""
    p = t64(part)
    if defect == 'drop_slot':
        p = p[:, :-1]
    tot = p.sum(1) / (HW * cg)
    mean = tot[..., 0]
    var = tot[..., 1] - mean * mean
    return mean, var, 1.0 / torch.sqrt(var.clamp_min(0) + eps)


def rstd_bound(c, mean, var, eps=EPS):
    """the variance rule: |rstd error| / rstd <= 1/2 c 2^-24 (mean^2 + var) / (var + eps) + 2^-23"""
    var = var.clamp_min(0)
    return 0.5 * c * U * (mean * mean + var) / (var + eps) + 2.0 ** -23


def mean_bound(c, mean, var):
    return c * U * (mean.abs() + var.clamp_min(0).sqrt())


def stats_within(mean_c, scale_c, x, gamma, row, c_mean, c_gn, defect=None):
    """-> (ok, worst mean error / bound, worst scale error / bound) of a kernel's (or a defective reference's) [n][C] outputs"""
    C, groups, HW = row
    mean, var, rstd = gn_ref(x, STATS_N, HW, C, groups)
    if defect is not None:
        dm, _, dr = gn_ref(x, STATS_N, HW, C, groups, defect=defect)
        mean_c, scale_c = gn_channels(dm, dr, gamma, C)
    cg = C // groups
    rm, rs = gn_channels(mean, rstd, gamma, C)
    bm = mean_bound(c_mean, mean, var).repeat_interleave(cg, 1)
    bs = (rstd_bound(c_gn, mean, var) * rstd).repeat_interleave(cg, 1) * t64(gamma).abs()
    em, es = (t64(mean_c) - rm).abs(), (t64(scale_c) - rs).abs()
    fin = bool(torch.isfinite(t64(mean_c)).all() and torch.isfinite(t64(scale_c)).all())
    wm = float(torch.where(bm > 0, em / bm.clamp_min(1e-300), torch.where(em == 0, 0.0, float('inf'))).max())
    ws = float(torch.where(bs > 0, es / bs.clamp_min(1e-300), torch.where(es == 0, 0.0, float('inf'))).max())
    return fin and wm <= 1.0 and ws <= 1.0, wm, ws


# ------------------------------------------------------------------ finalize
FIN_SLOTS = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1000)
FIN_N = (1, 33)
FIN_C = (64, 512)
# (n, nslots, C, groups).  With 32 groups the item count n x 32 fills whole blocks of both kernels (32 resp. 4 items each); the rows with
# 2 groups (66 resp. 2 items) end in a block that is partly empty
FIN_ROWS = [(n, ns, C, 32) for ns in FIN_SLOTS for (n, C) in ((1, 64), (33, 512), (33, 64), (1, 512))] + [
    (33, 7, 64, 2), (33, 513, 64, 2), (1, 9, 64, 2), (1, 1000, 64, 2)]


def finalize_inputs(row):
    """hand-built partials [n][nslots][groups][2] (mean ~ 0.3, var ~ 1, as test_hip_ops.py draws them), HW = 64 nslots; group 0 of image 0
    holds sums whose variance is slightly NEGATIVE (mean 2, E[x^2] = 4 (1 - 1e-4)) -> (part, gamma, HW)"""
    n, ns, C, groups = row
    g = torch.Generator().manual_seed(7 * n + 1000 * ns + C + groups)
    HW = 64 * ns
    cnt = 64.0 * (C // groups)
    s1 = torch.randn(n, ns, groups, generator=g) * cnt ** 0.5 + 0.3 * cnt
    s2 = (torch.rand(n, ns, groups, generator=g) + 0.5) * cnt + s1 * s1 / cnt
    s1[0, :, 0] = 2.0 * cnt
    s2[0, :, 0] = float(np.float32(4.0 * (1 - 1e-4) * cnt))
    gamma = torch.randn(C, generator=g)
    return torch.stack([s1, s2], -1).contiguous(), gamma, HW


def finalize_bounds(part, HW, cg, nslots):
    """the finalize adds in fp64: its two outputs carry their own fp32 rounding (mean: 2^-24 |mean|; scale: the rounding of rstd and of
    rstd gamma, 2^-23) plus the fp64 sum's error (nslots + 4 roundings of 2^-53 of the summed magnitude), which reaches rstd through the
    conditioning term of the variance rule -> (bound of |mean error|, bound of |rstd error| / rstd) [n][groups]"""
    p = t64(part)
    mag = p.abs().sum(1) / (HW * cg)
    mean, var, _ = finalize_ref(part, HW, cg)
    k = (nslots + 4) * 2.0 ** -53
    bm = U * mean.abs() + k * mag[..., 0]
    br = 2.0 ** -23 + 2.0 ** -46 + 0.5 * k * (mag[..., 1] + 2 * mean.abs() * mag[..., 0]) / (var.clamp_min(0) + EPS)
    return bm, br


# ------------------------------------------------------------------ apply
APPLY_ROWS = [(C, HW, 3) for C in (4, 128, 1024) for HW in (1, 63, 256)]
APPLY_LAP = (256, 16384, 3)                           # 3 x 16384 x 64 float4 > 8192 blocks x 256 threads: a second lap of the grid


def apply_inputs(row):
    """-> x rows [n HW][C], mean_c, scale_c [n][C] fp32 (per-image, a zero and negative scales among them), beta [C]"""
    C, HW, n = row
    s = 200003 + 31 * C + 13 * HW + n
    x = normal((n * HW, C), s, 3.0, 1.5)
    mean_c = normal((n, C), s + 1, 1.0, 1.5) + torch.arange(n, dtype=torch.float32).view(n, 1) * 3.0
    scale_c = normal((n, C), s + 2, 0.3, 0.6)
    scale_c[0, 0] = 0.0
    return x, mean_c, scale_c, normal((C,), s + 3, 0.2)


def apply_ref(x, mean_c, scale_c, beta, n, HW, C, swish_on, dtype=F64, defect=None):
    """-> (value, magnitude of t = (x - mean) scale + beta) rows [n HW][C].  Defect 'next_img': the statistics of image (img + 1) % n"""
    xv = x.to(dtype).view(n, HW, C)
    m, s = mean_c.to(dtype), scale_c.to(dtype)
    if defect == 'next_img':
        m, s = m.roll(-1, 0), s.roll(-1, 0)
    t = (xv - m.view(n, 1, C)) * s.view(n, 1, C) + beta.to(dtype).view(1, 1, C)
    mag = (xv.abs() + m.abs().view(n, 1, C)) * s.abs().view(n, 1, C) + beta.to(dtype).abs().view(1, 1, C)
    if swish_on:
        t = swish_f32(t) if dtype == torch.float32 else swish(t)
    return t.reshape(n * HW, C), mag.reshape(n * HW, C)


def apply_bound(c, ref, mag, swish_on, swish_u=SWISH_U):
    """c 2^-24 x magnitude of t; behind the swish that error grows by at most max |swish'| and the swish adds its own figure"""
    return c * U * mag * SWISH_LIP + swish_u * U * ref.abs() if swish_on else c * U * mag


def within(got, ref, bound):
    """-> (ok, worst |got - ref| / bound); an element of zero bound must match exactly, a non-finite result is infinitely far"""
    got, ref, bound = t64(got), t64(ref), t64(bound)
    if got.shape != ref.shape:
        return False, float('inf')
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float('inf')))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))
    w = float(r.max()) if r.numel() else 0.0
    return w <= 1.0, w


# ================================================================== GroupNorm prologue of the 1x1 GEMM
PRO_C = 128
# (rows_per_img, images, N, variant): variant 'full' = bias + residual, 'no_bias', 'no_res'.  M is a multiple of 128 on the first row only
PRO_ROWS = [(256, 3, 128, 'full'), (64, 3, 128, 'full'), (64, 5, 128, 'no_bias'), (192, 3, 128, 'full'), (192, 5, 128, 'no_res'),
            (48, 5, 128, 'full'), (48, 3, 128, 'no_bias'), (100, 3, 128, 'full'), (100, 5, 128, 'no_res'), (100, 5, 384, 'full')]
PRO_ARMS = ('f32', 'x6', 'x3h')
PRO_DEFECTS = ('row_off1', 'half_prev')


def pro_form(rpi):
    """the prologue instantiation gemm_x3h.hip picks (pro_rows_per_img % 128, % 64, neither)"""
    return 'img1' if rpi % 128 == 0 else 'img2' if rpi % 64 == 0 else 'generic'


def pro_inputs(row):
    """-> x rows [M][C] (image i centred at 3 i - 4), mean_c, scale_c [n][C] (float64 statistics rounded to fp32), beta, w [C][N], bias, res"""
    rpi, n, N, variant = row
    C, M = PRO_C, rpi * n
    s = 300007 + 31 * rpi + 17 * n + N
    x = normal((M, C), s, 1.5) + (torch.arange(M) // rpi).float().view(M, 1) * 3.0 - 4.0
    gamma, beta = normal((C,), s + 1, 0.3, 1.0), normal((C,), s + 2, 0.2)
    mean, _, rstd = gn_ref(x, n, rpi, C, 32)
    mc, sc = gn_channels(mean, rstd, gamma, C)
    w, b, res = normal((C, N), s + 3, 0.05), normal((N,), s + 4), normal((M, N), s + 5)
    return x, mc.float(), sc.float(), beta, w, (None if variant == 'no_bias' else b), (None if variant == 'no_res' else res)


def pro_activation(x, mean_c, scale_c, beta, rpi, swish_on, dtype=F64, defect=None):
    """the prologue on rows: -> (a, magnitude of t) [M][C].  Defects: 'row_off1' = the image of row m + 1 (wrong on the last row of an
    image); 'half_prev' = rows 64 .. 127 of a 128-row tile take the image of the row 64 above them"""
    M, C = x.shape
    m = torch.arange(M)
    img = m // rpi
    if defect == 'row_off1':
        img = ((m + 1) // rpi).clamp(max=mean_c.shape[0] - 1)
    if defect == 'half_prev':
        img = torch.where(m % 128 >= 64, (m - 64) // rpi, img)
    xv, mu, sc, be = x.to(dtype), mean_c.to(dtype)[img], scale_c.to(dtype)[img], beta.to(dtype).view(1, C)
    t = (xv - mu) * sc + be
    mag = (xv.abs() + mu.abs()) * sc.abs() + be.abs()
    if swish_on:
        t = swish_f32(t) if dtype == torch.float32 else swish(t)
    return t, mag


def pro_ref(row, inputs, swish_on, defect=None):
    """-> (value, conv magnitude |a| |w| + |b| + |res|, MAG = that + the prologue's own magnitude carried through |w|)"""
    x, mc, sc, beta, w, b, res = inputs
    a, magt = pro_activation(x, mc, sc, beta, row[0], swish_on, defect=defect)
    w6 = t64(w)
    ref, mag = a @ w6, a.abs() @ w6.abs()
    if b is not None:
        ref, mag = ref + t64(b), mag + t64(b).abs()
    if res is not None:
        ref, mag = ref + t64(res), mag + t64(res).abs()
    return ref, mag, mag + (magt * (SWISH_LIP if swish_on else 1.0)) @ w6.abs()


def pro_f32(row, inputs, swish_on):
    x, mc, sc, beta, w, b, res = inputs
    a, _ = pro_activation(x, mc, sc, beta, row[0], swish_on, dtype=torch.float32)
    y = seq_matmul_f32(a, w)
    if b is not None:
        y = y + b
    return y + res if res is not None else y


def pro_bound(c, mag, MAG, swish_on, swish_u):
    return c * U * MAG + (swish_u * U * mag if swish_on else 0.0)


# ================================================================== spatial attention
ATTN_SHAPES = [(256, 256), (64, 512), (64, 256)]      # (HW, C): every accepted pair
ATTN_N = (1, 3)
ATTN_CLASSES = ('exact', 'selector', 'shifted', 'shifted100', 'random')
ATTN_SELECT_A = 2.0                                   # gap a^2 sqrt(C) = 64 (C = 256) / 90.5 (C = 512) > 60; |q|, |k| = 2: inside the x3h arm's range
# every score + 80 (fp32 exp(s) itself still fits: 256 e^81 < 2^128) and + 100 (e^100 does not: a kernel without max-subtraction overflows)
ATTN_SHIFTS = {'shifted': 80.0, 'shifted100': 100.0}


def hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def attn_perm(HW):
    return rng(41 + HW).permutation(HW)


def attn_inputs(cls, HW, C, n):
    """-> q, k, v float32 [n][HW][C]"""
    s = 400009 + 31 * HW + 17 * C + n + 1000 * ATTN_CLASSES.index(cls)
    if cls == 'exact':                                # uniform softmax over HW = 2^8 / 2^6 keys of small integers
        q = torch.zeros((n, HW, C))
        v = torch.from_numpy(rng(s).integers(-8, 9, size=(n, HW, C)).astype(np.float32))
        return q, normal((n, HW, C), s + 1, 0.7), v
    if cls == 'selector':
        u = torch.from_numpy(hadamard(C)[:HW].astype(np.float32)) * ATTN_SELECT_A
        k = u.expand(n, HW, C).contiguous()
        q = u[torch.from_numpy(attn_perm(HW))].expand(n, HW, C).contiguous()
        return q, k, normal((n, HW, C), s + 2)
    q, k, v = (normal((n, HW, C), s + i, 0.7) for i in (3, 4, 5))
    if cls in ATTN_SHIFTS:                            # channel 0 of q and k is the constant A: every score + A^2 scale = the shift
        A = float(np.float32((ATTN_SHIFTS[cls] * C ** 0.5) ** 0.5))
        q[:, :, 0] = A
        k[:, :, 0] = A
    return q, k, v


def attn_scale(C):
    return float(np.float32(C ** -0.5))


def attn_ref(q, k, v, scale, defect=None):
    """softmax(q k^T scale) v per image -> (out [n][HW][C], M = sum_j p |v|, S [n][HW] = max_j scale sum_c |q| |k|, p, scores).
    Defects: 'drop_tile' = the last 32 keys are not seen; 'no_scale'"""
    q, k, v = t64(q), t64(k), t64(v)
    if defect == 'drop_tile':
        k, v = k[:, :-32], v[:, :-32]
    sc = 1.0 if defect == 'no_scale' else scale
    s = q @ k.transpose(1, 2) * sc
    p = torch.softmax(s, -1)
    S = (q.abs() @ k.abs().transpose(1, 2) * sc).max(-1).values
    return p @ v, p @ v.abs(), S, p, s


def attn_pack(q, k, v, ld):
    """the fused projection's layout: rows [n HW][ld] = q | k | v | gap, the gap holding NaN"""
    n, HW, C = q.shape
    buf = torch.full((n * HW, ld), float('nan'))
    buf[:, :3 * C] = torch.cat([q, k, v], -1).view(n * HW, 3 * C)
    return buf


def attn_unpack(buf, n, HW, C, ld):
    """rows of leading dimension ``ld`` read from the flat buffer (``ld`` = 3 C on a wider buffer: the 'ld' defect)"""
    flat = buf.reshape(-1)[:n * HW * ld].view(n * HW, ld)
    return tuple(flat[:, i * C:(i + 1) * C].reshape(n, HW, C) for i in range(3))


def attn_f32(q, k, v, scale):
    """float32 restatement: scores as one chain over the channels, softmax over all keys at once, P V as one chain over the keys
    -> (out, scores)"""
    s = seq_matmul_f32(q, k.transpose(1, 2).contiguous()) * torch.tensor(scale, dtype=torch.float32)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    return seq_matmul_f32(p, v), s


def attn_score_key(cls):
    """which calibration constant the scores of a class take"""
    return 'attn_s_shift' if cls in ATTN_SHIFTS else 'attn_s'


def attn_bound(c_pv, c_s, M, S):
    """c_pv 2^-24 M for the softmax and P V, plus what a score error of c_s 2^-24 S does to the probabilities (each moves by at most
    twice the largest score error, relatively)"""
    return U * M * (c_pv + 2.0 * c_s * S.unsqueeze(-1))


# ================================================================== codebook
CB_SHAPES = [(32, 64), (256, 1024), (64, 200), (32, 257)]        # (D, Kc)
# (M, D, Kc): M = 1, 127, 128, 129, 385 against every codebook
LOOKUP_ROWS = [(1, 32, 64), (129, 32, 64), (127, 64, 200), (128, 64, 200), (385, 64, 200), (127, 32, 257), (128, 32, 257), (385, 32, 257),
               (129, 256, 1024), (385, 256, 1024)]
TAU_C = 16.0


def codebook(D, Kc):
    return normal((D, Kc), 500009 + 31 * D + Kc, 0.3)


def colsumsq_f32(E):
    acc = torch.zeros(E.shape[1], dtype=torch.float32)
    for d in range(E.shape[0]):
        acc = acc + E[d] * E[d]
    return acc


def gather_indices(Kc, M=37):
    idx = torch.from_numpy(rng(61 + Kc).integers(0, Kc, size=M))
    idx[3], idx[11], idx[0], idx[M - 1] = -5, Kc + 3, 0, Kc - 1
    return idx


def gather_ref(E, idx, defect=None):
    """rows E[:, clamp(idx)]; defect 'unclamped': the index taken modulo Kc (what a wrapped read returns)"""
    Kc = E.shape[1]
    i = idx % Kc if defect == 'unclamped' else idx.clamp(0, Kc - 1)
    return E.t()[i].contiguous()


def dist64(z, E):
    """|z|^2 - 2 z E + |e|^2 in float64 [M][Kc], the reference's own statement of the distance"""
    z, E = t64(z), t64(E)
    return z.pow(2).sum(1, keepdim=True) - 2.0 * (z @ E) + E.pow(2).sum(0, keepdim=True)


def planted_inputs(row):
    """z = E[:, k] + noise with |noise| <= 1 % of the smallest distance between two codes -> (z [M][D], E, k [M]); the chosen k include
    the last code of a ragged 128-code tile, the first code of the next tile and Kc - 1"""
    M, D, Kc = row
    E = codebook(D, Kc)
    g = rng(600011 + 31 * M + 17 * D + Kc)
    k = g.integers(0, Kc, size=M)
    must = list(dict.fromkeys(c for c in (Kc - 1, 127, 128, (Kc - 1) // 128 * 128, (Kc - 1) // 128 * 128 - 1, 0, 255, 256) if 0 <= c < Kc))
    k[:min(M, len(must))] = must[:M]
    Et = t64(E).t()
    dd = torch.cdist(Et, Et)
    dd.fill_diagonal_(float('inf'))
    dmin = float(dd.min())
    noise = g.standard_normal(size=(M, D))
    noise = noise / np.linalg.norm(noise, axis=1, keepdims=True) * (0.01 * dmin * g.uniform(0.2, 1.0, size=(M, 1)))
    z = (Et[torch.from_numpy(k)].numpy() + noise).astype(np.float32)
    return torch.from_numpy(z), E, torch.from_numpy(k), dmin


def random_lookup_inputs(row):
    M, D, Kc = row
    return normal((M, D), 700001 + 31 * M + 17 * D + Kc, 0.3), codebook(D, Kc)


def lookup_tau(z, E):
    """tau = 16 x 2^-24 (|z|^2 + max |e|^2) per row"""
    return TAU_C * U * (t64(z).pow(2).sum(1) + float(t64(E).pow(2).sum(0).max()))


def lookup_check(idx, z, E):
    """random class -> (ok, exempt share, message): equal to the float64 argmin but where the float64 margin between best and second
    best is below tau; there one of the codes within tau of the minimum"""
    d = dist64(z, E)
    best = d.min(1)
    two = d.topk(2, 1, largest=False).values
    tau = lookup_tau(z, E)
    exempt = (two[:, 1] - two[:, 0]) < tau
    idx = idx.long()
    inr = bool(((idx >= 0) & (idx < E.shape[1])).all())
    if not inr:
        return False, float(exempt.double().mean()), 'an index outside [0, Kc)'
    wrong = (idx != best.indices) & ~exempt
    far = exempt & (d.gather(1, idx.view(-1, 1)).view(-1) - best.values > tau)
    return not bool(wrong.any() or far.any()), float(exempt.double().mean()), f'{int(wrong.sum())} wrong rows, {int(far.sum())} exempt rows outside tau'


def tie_inputs():
    """Kc = 257, D = 32: duplicate codes (5, 256) across two code tiles, (7, 200), (129, 130) in neighbouring lanes, (40, 72) in one lane;
    the eight query rows sit on both half-waves (rows 0-3 / 4-7) -> (z, E, expected)"""
    E = codebook(32, 257)
    for a, b in ((5, 256), (7, 200), (129, 130), (40, 72)):
        E[:, b] = E[:, a]
    z = torch.stack([E[:, c] for c in (7, 129, 200, 5, 256, 40, 72, 130)], 0).contiguous()
    return z, E, [7, 129, 7, 5, 5, 40, 40, 129]


def argmin_ref(z, E, defect=None):
    """float64 argmin, ties to the lowest index; defect 'tie_high': to the highest"""
    d = dist64(z, E)
    lo = d.min(1, keepdim=True).values
    cand = (d <= lo + 1e-12 * (1 + lo.abs())).double()                               # (duplicate codes: equal up to the float64 GEMM's blocking)
    if defect == 'tie_high':
        return (d.shape[1] - 1) - cand.flip(1).argmax(1)
    return cand.argmax(1)


# ================================================================== conv_in
CONV_IN_ROWS = [(4, 1, 1, 1), (32, 2, 5, 7), (128, 3, 9, 17), (256, 1, 8, 24), (64, 2, 1, 33)]          # (Cout, n, H, W)
CONV_IN_LAPS = [(32, 5, 256, 256), (128, 9, 256, 256)]            # past 8192 x 256 threads of 4 channels / 16384 x 256 of 16
CONV_IN_X3H_ROWS = [(1, 8, 16, 128), (3, 24, 16, 128), (2, 8, 48, 256)]                                # (n, H, W, Cout)


def preprocess_u8(img):
    """the kernel's fp32 pre-processing of a byte: (u8 (1 / 255)) 2 - 1, each step rounded to float32"""
    return (img.float() * torch.tensor(1.0 / 255, dtype=torch.float32)) * 2 - 1


def conv_in_inputs(row):
    """-> img uint8 [n][H][W][3], w [Cout][3][3][3], bias"""
    cout, n, H, W = row
    s = 800003 + 31 * cout + 17 * n + 13 * H + W
    img = torch.from_numpy(rng(s).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8))
    return img, normal((cout, 3, 3, 3), s + 1, 0.2), normal((cout,), s + 2)


def conv_in_ref(img, w, bias, defect=None):
    """float64 convolution of the fp32-pre-processed image -> (value, magnitude) NHWC [n][H][W][Cout].
    Defects: 'div256' = u8 / 256 in place of / 255; 'taps' = ky <-> kx"""
    x = (img.double() / 256 * 2 - 1) if defect == 'div256' else preprocess_u8(img).double()
    x, w6 = x.permute(0, 3, 1, 2), t64(w)
    if defect == 'taps':
        w6 = w6.transpose(2, 3)
    ref, mag = F.conv2d(x, w6, padding=1), F.conv2d(x.abs(), w6.abs(), padding=1)
    if bias is not None:
        ref, mag = ref + t64(bias).view(1, -1, 1, 1), mag + t64(bias).abs().view(1, -1, 1, 1)
    return ref.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def conv_in_f32(img, w, bias):
    """the kernel's order: bias, then (ky, kx, ci) as one float32 chain"""
    x = F.pad(preprocess_u8(img), (0, 0, 1, 1, 1, 1))                                # NHWC, zero border
    n, H, W = img.shape[:3]
    acc = (bias if bias is not None else torch.zeros(w.shape[0])).float().expand(n, H, W, w.shape[0])
    for ky in range(3):
        for kx in range(3):
            for ci in range(3):
                acc = acc + x[:, ky:ky + H, kx:kx + W, ci, None] * w[:, ci, ky, kx].view(1, 1, 1, -1)
    return acc


# ================================================================== conv3_small_cout
SMALL_ROWS = [(32, 1, 1, 8, 32), (96, 2, 3, 16, 32), (128, 3, 2, 8, 64), (672, 4, 1, 8, 32), (672, 3, 2, 16, 64)]    # (Cin, Cout, n, H, W)
SMALL_PRO = (None, 'lin', 'swish')
SMALL_REFUSED = [(704, 3, 1, 8, 32), (48, 3, 1, 8, 32), (32, 5, 1, 8, 32), (32, 3, 1, 12, 32), (32, 3, 1, 8, 48)]


def small_seed(row):
    cin, cout, n, H, W = row
    return 900001 + 31 * cin + 17 * cout + 13 * H + 11 * W + 5 * n


def small_inputs(row, bf16):
    """-> x NCHW (``bf16``: values exact in bf16), w, bias, mean_c, scale_c [n][Cin] (float64 statistics of x rounded to fp32; image i
    centred at i - 0.5), beta"""
    cin, cout, n, H, W = row
    s = small_seed(row)
    x = normal((n, cin, H, W), s, 1.4) + torch.arange(n).float().view(n, 1, 1, 1) - 0.5
    if bf16:
        x = x.to(torch.bfloat16).float()
    gamma, beta = normal((cin,), s + 3, 0.3, 1.0), normal((cin,), s + 4, 0.2)
    mean, _, rstd = gn_ref(CR.to_rows(x), n, H * W, cin, 32)
    mc, sc = gn_channels(mean, rstd, gamma, cin)
    return x, normal((cout, cin, 3, 3), s + 1, 0.05), normal((cout,), s + 2), mc.float(), sc.float(), beta


def small_exact_inputs(row):
    """integers in [-4, 4] x multiples of 2^-2: every partial sum is exact in fp32 (672 x 9 x 4 / 2^-2 < 2^22)"""
    cin, cout, n, H, W = row
    return CR.exact_inputs(('s1', cin, cout, H, W, n))[:3]


def small_ref(x, w, bias, pro, swish_on, defect=None):
    """-> (value, conv magnitude, MAG) rows [n H W][Cout]; ``pro`` = (mean_c, scale_c, beta) or None.  Defects: 'drop_chunk' = the last 32
    input channels are not summed; 'pro_pad' = the prologue is applied to the zero padding too"""
    n, cin, H, W = x.shape
    a, magt = t64(x), None
    if pro is not None:
        mc, sc, beta = pro
        a = CR.prologue(x, mc, sc, beta, swish_on)
        magt = (t64(x).abs() + t64(mc).abs().view(n, cin, 1, 1)) * t64(sc).abs().view(n, cin, 1, 1) + t64(beta).abs().view(1, cin, 1, 1)
    w6 = t64(w)
    if defect == 'drop_chunk':
        w6 = w6.clone()
        w6[:, -32:] = 0.0
    if defect == 'pro_pad' and pro is not None:
        big = CR.prologue(F.pad(t64(x), (1, 1, 1, 1)), mc, sc, beta, swish_on)
        ref = CR.to_rows(F.conv2d(big, w6))
    else:
        ref = CR.to_rows(F.conv2d(a, w6, padding=1))
    mag = CR.to_rows(F.conv2d(a.abs(), w6.abs(), padding=1))
    MAG = mag if magt is None else mag + CR.to_rows(F.conv2d(magt * (SWISH_LIP if swish_on else 1.0), t64(w).abs(), padding=1))
    if bias is not None:
        ref, mag, MAG = ref + t64(bias), mag + t64(bias).abs(), MAG + t64(bias).abs()
    return ref, mag, MAG


def small_f32(x, w, bias, pro, swish_on):
    """the kernel's order: bias, then (chunk, tap, channel) as one float32 chain per output"""
    n, cin, H, W = x.shape
    a = x.float()
    if pro is not None:
        a = CR.prologue(x, pro[0], pro[1], pro[2], False, dtype=torch.float32)
        a = swish_f32(a) if swish_on else a
    ap = F.pad(a, (1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous().numpy()              # [n][H + 2][W + 2][Cin]
    wn = w.float().numpy()
    acc = np.zeros((n, H, W, w.shape[0]), dtype=np.float32) + (bias.float().numpy() if bias is not None else np.float32(0))
    for chunk in range(cin // 32):
        for tap in range(9):
            ky, kx = tap // 3, tap % 3
            sl = ap[:, ky:ky + H, kx:kx + W]
            for c in range(chunk * 32, chunk * 32 + 32):
                acc = acc + sl[..., c, None] * wn[:, c, ky, kx]
    return torch.from_numpy(acc.reshape(n * H * W, -1))
