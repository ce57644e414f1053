"""Test infrastructure of the per-kernel tests of the transformer's (MIGT) row kernels
(tests/test_hip_transformer_kernels.py on the GPU, tests/test_transformer_kernels_ref_host.py on the CPU), built like
tests/training_kernels_ref.py and on its helpers.

For every kernel: a float64 restatement written from the operation's definition, returning ``(value, magnitude)``: the magnitude is the
same expression with every summand replaced by its absolute value and None where the kernel is in the exact class (copies, selections,
sums of three dyadic numbers, integer results).  Two magnitudes are not a literal application of that rule, and say so where they are
formed: a softmax probability is judged against p (1 + |z - max z|) because exp turns the rounding of its argument, |z - max z| 2^-24,
into that relative error of the result, and a GELU output against the magnitude of its argument because |gelu'| <= 1.13 and
|gelu(a)| <= |a|.  ``*_f32`` functions restate the KERNEL's formula on torch-CPU float32 (sums that the kernel splits into partial sums
in the kernel's order): the host test measures their distance from float64 on the very inputs of the GPU test and the GPU test's
constants come from that measurement, never from the kernel.  Scalars reach a kernel as float32: the references take them as Python
floats and the callers hand over the float32 values (``f32``).  The references run on the device of their inputs (the second-lap cases
hand over device tensors).  Input generators and case lists live here so that both files see the same tensors."""
import math

import numpy as np
import torch

from training_kernels_ref import U, F64, t64, rng, dyadic, normal, SOFTMAX_CASES  # noqa: F401  (one definition of each, shared)

F32 = torch.float32
RSQRT2 = 0.70710678118654752440
RSQRT2PI = 0.39894228040143267794
F32_TINY = 2.0 ** -126                                # float32's smallest normal number


def f32(v):
    """the float32 value a scalar argument has inside a kernel, as a Python float"""
    return float(np.float32(v))


def _t32(v):
    return torch.tensor(v, dtype=F32)


# ------------------------------------------------------------------ exact class
TRANSPOSE_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (70, 45)]
TRANSPOSE_VARIANTS = [(batch, pad, bf16) for batch in (1, 3) for pad in ((0, 0), (3, 5)) for bf16 in (False, True)]


def transpose_input(rows, cols, batch, pad_src, bf16):
    """[batch][rows][cols + pad_src] on the dyadic grid; a bf16 source holds the bf16 roundings of the grid (widening them is exact)"""
    x = dyadic((batch, rows, cols + pad_src), 300 + 7 * rows + cols + batch, ties=False)
    return x.bfloat16() if bf16 else x


def transpose(src, rows, cols):
    """dst[b][c][r] = src[b][r][c] for r < rows, c < cols"""
    return t64(src.float())[:, :rows, :cols].transpose(1, 2).contiguous(), None


EMBED_CASES = [(1, 1, 4, 1), (6, 16, 128, 66), (3, 50, 2048, 10)]


def embed_inputs(BS, L, d, V):
    g = rng(320 + d + V)
    ids = g.integers(0, V, size=(BS, L)).astype(np.int32)
    ids.reshape(-1)[0] = 0
    ids.reshape(-1)[-1] = V - 1
    return torch.from_numpy(ids), dyadic((V, d), 321 + d), dyadic((L, d), 322 + d), dyadic((BS, d), 323 + d)


def embed_sum(ids, wte, wpe, add, BS, L, d):
    """out[bs][l] = (wte[ids[bs][l]] + wpe[l]) + add[bs]: three multiples of 2^-6 below 8, exact in float32 in any order"""
    return ((t64(wte)[ids.long()] + t64(wpe)[None]) + t64(add)[:, None]).reshape(BS * L, d), None


ARGMAX_N = [1, 63, 64, 65, 1024, 1026]
ARGMAX_KINDS = ['plain', 'tie_next_lane', 'tie_same_lane', 'all_equal', 'all_neg_inf', 'pos_inf']
ARGMAX_PAD = 4


def argmax_input(rows, n, kind):
    """[rows][n + 4] with +3e38 in the four pad columns (a read past n wins the row).  ``tie_next_lane``: the row maximum at columns
    c and c + 1, ``tie_same_lane``: at c and c + 64 (one lane of the wave walks both), c differing from row to row; a kind the row is too
    short for leaves the plain grid, whose own maxima repeat (1025 levels)"""
    x = dyadic((rows, n + ARGMAX_PAD), 340 + 3 * rows + n)
    for r in range(rows):
        c = (37 * r + n // 3) % n
        if kind == 'tie_next_lane' and n >= 2:
            c = min(c, n - 2)
            x[r, c] = x[r, c + 1] = 9.0
        elif kind == 'tie_same_lane' and n >= 65:
            c = c % (n - 64)
            x[r, c] = x[r, c + 64] = 9.0
        elif kind == 'all_equal':
            x[r, :n] = -2.5
        elif kind == 'all_neg_inf':
            x[r, :n] = -math.inf
        elif kind == 'pos_inf':
            x[r, c] = math.inf
    x[:, n:] = 3e38
    return x


def argmax_rows(x, n):
    """the smallest column that holds the row's maximum"""
    v = t64(x)[:, :n]
    col = torch.arange(n, device=v.device)
    return torch.where(v == v.max(1, keepdim=True).values, col, n).min(1).values, None


def argmax_rows_last(x, n):
    """the mistake: a tie resolved to the higher column"""
    v = t64(x)[:, :n]
    col = torch.arange(n, device=v.device)
    return torch.where(v == v.max(1, keepdim=True).values, col, -1).max(1).values


POSTPROCESS_BIG = 16384 * 256 + 5                     # one element more than the capped grid covers: the loop's second lap


def postprocess_input():
    """around every threshold x_k = 2 k / 255.5 - 1 (k = 1 .. 255) at which the uint8 result steps: the float32 nearest to it and its two
    neighbours on either side; and -3, -1, -0.0, 0, 1, 7"""
    k = np.arange(1, 256, dtype=np.float64)
    c = (2.0 * k / 255.5 - 1.0).astype(np.float32)
    lo1, hi1 = np.nextafter(c, np.float32(-2)), np.nextafter(c, np.float32(2))
    lo2, hi2 = np.nextafter(lo1, np.float32(-2)), np.nextafter(hi1, np.float32(2))
    v = np.stack((lo2, lo1, c, hi1, hi2), 1).reshape(-1)
    return torch.from_numpy(np.concatenate((v, np.array([-3.0, -1.0, -0.0, 0.0, 1.0, 7.0], np.float32))))


def postprocess_u8(x):
    """clip to [-1, 1], / 2 + 0.5, times 255.5 and truncate, every step in float32 as the operation is defined (the thresholds are where
    the float32 product crosses an integer, so float64 is not the reference here; oracle.vqgan_oracle.postprocess_u8 is)"""
    v = x.to(F32).clamp(-1.0, 1.0) / 2.0 + 0.5
    return (v * torch.tensor(255.5, dtype=F32, device=v.device)).to(torch.int32).clamp(0, 255).to(torch.uint8), None


# ------------------------------------------------------------------ column sums
COLSUM_CASES = [(1, 1, 1), (127, 64, 64), (128, 66, 68), (129, 256, 256), (1000, 260, 260), (1000, 130, 130), (32773, 260, 264)]
COLSUM_PAD = 1e30


def colsum_inputs(M, N, ld):
    """x [M][ld] with 1e30 in the columns from N on (a pad column read into a sum shows), out0 the non-zero start of the accumulation"""
    x = normal((M, ld), 400 + M % 1000 + N)
    x[:, N:] = COLSUM_PAD
    return x, normal((N,), 401 + N)


def colsum(x, out0, M, N, accumulate):
    v = t64(x)[:, :N]
    s, a = v.sum(0), v.abs().sum(0)
    return (t64(out0) + s, t64(out0).abs() + a) if accumulate else (s, a)


def colsum_f32(x, out0, M, N, ld, accumulate):
    """the kernel's order: at most 256 splits of ceil(M / nsplit) rows; inside a split one running sum per row phase (four phases, combined
    as (0 + 1) + (2 + 3)) in the float4 kernel, one running sum in the one-column-per-thread kernel (ld no multiple of 4, or N < 64); the
    splits are added in order, out0 last"""
    nsplit = min(256, (M + 127) // 128)
    per = (M + nsplit - 1) // nsplit
    v = torch.zeros((nsplit * per, N), dtype=F32)
    v[:M] = x.float()[:, :N]
    v = v.view(nsplit, per, N)
    if (ld & 3) or N < 64:
        part = torch.zeros((nsplit, N), dtype=F32)
        for m in range(per):
            part = part + v[:, m]
    else:
        steps = (per + 3) // 4
        w = torch.zeros((nsplit, steps * 4, N), dtype=F32)
        w[:, :per] = v
        w = w.view(nsplit, steps, 4, N)
        ph = torch.zeros((nsplit, 4, N), dtype=F32)
        for k in range(steps):
            ph = ph + w[:, k]
        part = (ph[:, 0] + ph[:, 1]) + (ph[:, 2] + ph[:, 3])
    s = torch.zeros(N, dtype=F32)
    for i in range(nsplit):
        s = s + part[i]
    return out0.float() + s if accumulate else s


# ------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-5
LN_D = [4, 252, 256, 260, 512, 516, 1024, 1028, 2048]
LN_ROWS = [1, 5]


def ln_inputs(rows, d):
    """with five rows: row 1 constant (variance 0: rstd = 1 / sqrt(eps)), row 2 of mean 100 and std 0.01 (the mean's rounding is what is
    left of x - mean)"""
    x = normal((rows, d), 420 + rows + d, 2.0, 0.3)
    if rows >= 3:
        x[1] = 1.5
        x[2] = normal((d,), 421 + d, 0.01, 100.0)
    return x, normal((d,), 422 + d, 0.3, 1.0), normal((d,), 423 + d, 0.2, 0.1)


def _ln_stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def layernorm(x, gamma, beta, eps):
    """(x - mean) rstd gamma + beta with the biased variance; magnitude (|x| + mean|x|) rstd |gamma| + |beta|"""
    x, g, b = t64(x), t64(gamma), t64(beta)
    mean, rstd = _ln_stats(x, eps)
    return (x - mean) * rstd * g + b, (x.abs() + x.abs().mean(-1, keepdim=True)) * rstd * g.abs() + b.abs()


def _ln_stats_f32(x, eps):
    d = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / d
    t = x - mean
    return t, 1.0 / torch.sqrt((t * t).sum(-1, keepdim=True) / d + _t32(eps))


def layernorm_f32(x, gamma, beta, eps):
    t, rstd = _ln_stats_f32(x.float(), eps)
    return t * rstd * gamma.float() + beta.float()


LN_BWD_CASES = [(37, d) for d in (4, 256, 260, 512, 516, 768, 772, 1024)] + [(rows, 260) for rows in (1, 3, 16, 17, 33)]
LN_BWD_VARIANTS = [(accumulate, res) for accumulate in (False, True) for res in (False, True)]
LN_BWD_RPB = 16                                       # rows per block of the backward kernel: four waves, each walks every fourth row


def ln_bwd_inputs(rows, d):
    s = 440 + 3 * rows + d
    return (normal((rows, d), s), normal((rows, d), s + 1, 2.0, 0.3), normal((d,), s + 2, 0.3, 1.0), normal((rows, d), s + 3),
            normal((d,), s + 4), normal((d,), s + 5))


def layernorm_bwd(dy, x, gamma, eps, res=None, dg0=None, db0=None):
    """g = dy gamma, xhat = (x - mean) rstd: dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ res], dgamma [dg0 +] sum_r dy xhat,
    dbeta [db0 +] sum_r dy -> ((dx, dgamma, dbeta), magnitudes)"""
    dy, x, gm = t64(dy), t64(x), t64(gamma)
    mean, rstd = _ln_stats(x, eps)
    xh = (x - mean) * rstd
    xa = (x.abs() + x.abs().mean(-1, keepdim=True)) * rstd
    g, ga = dy * gm, dy.abs() * gm.abs()
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    mx = rstd * (ga + ga.mean(-1, keepdim=True) + xa * (ga * xa).mean(-1, keepdim=True))
    dg, mg, db, mb = (dy * xh).sum(0), (dy.abs() * xa).sum(0), dy.sum(0), dy.abs().sum(0)
    if res is not None:
        dx, mx = dx + t64(res), mx + t64(res).abs()
    if dg0 is not None:
        dg, mg, db, mb = t64(dg0) + dg, t64(dg0).abs() + mg, t64(db0) + db, t64(db0).abs() + mb
    return (dx, dg, db), (mx, mg, mb)


def _rows_in_kernel_order(t):
    """sum over rows as the backward kernel forms it: per block of 16 rows wave w adds rows w, w + 4, w + 8, w + 12 in turn, the waves
    combine as (0 + 1) + (2 + 3), the blocks by a butterfly (b0 + b1) + (b2 + b3) ..."""
    rows, d = t.shape
    nb = (rows + LN_BWD_RPB - 1) // LN_BWD_RPB
    v = torch.zeros((nb * LN_BWD_RPB, d), dtype=F32)
    v[:rows] = t
    v = v.view(nb, 4, 4, d)                            # [block][step][wave]
    w = torch.zeros((nb, 4, d), dtype=F32)
    for k in range(4):
        w = w + v[:, k]
    parts = list(((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])).unbind(0))
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def layernorm_bwd_f32(dy, x, gamma, eps, res=None, dg0=None, db0=None):
    dy, x, gm = dy.float(), x.float(), gamma.float()
    d = x.shape[-1]
    t, rstd = _ln_stats_f32(x, eps)
    xh = t * rstd
    g = dy * gm
    dx = rstd * (g - g.sum(-1, keepdim=True) / d - xh * ((g * xh).sum(-1, keepdim=True) / d))
    dg, db = _rows_in_kernel_order(dy * xh), _rows_in_kernel_order(dy)
    if res is not None:
        dx = dx + res.float()
    if dg0 is not None:
        dg, db = dg0.float() + dg, db0.float() + db
    return dx, dg, db


# ------------------------------------------------------------------ GELU (exact erf)
GELU_SIZES = [1, 1028, 32768 * 256 + 5]               # the last: one block more than the capped grid covers (second lap), on the device


def gelu_sweep():
    """[-12, 12] in steps of 2^-6, and 0, -0.0, +/-1e-30"""
    return torch.cat((torch.arange(-768, 769, dtype=F32) / 64.0, torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=F32)))


def gelu_inputs(n, device='cpu', sweep=None):
    """u: element i is sweep value (1021 i + 700) mod 1541 (1021 is prime to 1541 = 23 x 67: 1541 consecutive elements hold the whole
    sweep; element 0 is -1.0625); df: a generator's normals on ``device``"""
    sw = (gelu_sweep() if sweep is None else sweep).to(device)
    i = torch.arange(n, device=device)
    u = sw[(i * 1021 + 700) % sw.numel()]
    if str(device) == 'cpu':
        return u, normal((n,), 460 + n % 997)
    return u, torch.randn((n,), generator=torch.Generator(device=device).manual_seed(460), device=device)


def gelu(u):
    """0.5 u (1 + erf(u / sqrt 2)); magnitude 0.5 |u| (1 + |erf|): the cancellation of 1 + erf at negative u is the kernel's to lose"""
    u = t64(u)
    e = torch.erf(u * RSQRT2)
    return 0.5 * u * (1.0 + e), 0.5 * u.abs() * (1.0 + e.abs())


def gelu_f32(u):
    u = u.float()
    return _t32(0.5) * u * (1.0 + torch.erf(u * _t32(RSQRT2)))


def gelu_bwd(u, df):
    """df (Phi(u) + u phi(u)), Phi = 0.5 (1 + erf(u / sqrt 2)), phi = exp(-u^2 / 2) / sqrt(2 pi)"""
    u, df = t64(u), t64(df)
    e = torch.erf(u * RSQRT2)
    pdf = RSQRT2PI * torch.exp(-0.5 * u * u)
    return df * (0.5 * (1.0 + e) + u * pdf), df.abs() * (0.5 * (1.0 + e.abs()) + u.abs() * pdf)


def gelu_bwd_f32(u, df):
    u, df = u.float(), df.float()
    cdf = _t32(0.5) * (1.0 + torch.erf(u * _t32(RSQRT2)))
    pdf = _t32(RSQRT2PI) * torch.exp(_t32(-0.5) * (u * u))
    return df * (u * pdf + cdf)


ERF_AS_ERR = 1.5e-7                                   # |erf error| of Abramowitz & Stegun 7.1.26 as csrc/vf_common.h states it


def gelu_bwd_bf16_bound(want, df):
    """the bf16-output backward is judged against 2^-9 |want| + 1.5e-7 |df| (a bf16 rounding; the stated error of the erf approximation
    times the incoming gradient) -> that bound in the helper's unit, as a magnitude: bound / 2^-24"""
    return (2.0 ** -9 * t64(want).abs() + ERF_AS_ERR * t64(df).abs()) / U


def gelu_bwd_fast_f32(u, df):
    """vf_gelu_grad_fast on float32: erf by Abramowitz & Stegun 7.1.26 with exp(-z^2) as exp2, the Gaussian from the same exponential;
    times df, rounded to bf16"""
    u, df = u.float(), df.float()
    z = u.abs() * _t32(RSQRT2)
    t = 1.0 / (_t32(0.3275911) * z + 1.0)
    p = _t32(1.061405429) * t + _t32(-1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + _t32(c)
    e = torch.exp2(_t32(-1.4426950408889634) * (z * z))
    erf_abs = 1.0 - (p * t) * e
    cdf = _t32(0.5) * (1.0 + torch.copysign(erf_abs, u))
    return (df * (u * (_t32(RSQRT2PI) * e) + cdf)).bfloat16()


# ------------------------------------------------------------------ softmax, the view masks
def _softmax(z):
    """softmax of float64 rows -> (p, magnitude p (1 + |z - max z|)): every term of the sum is positive, and exp carries the rounding of its
    argument, |z - max z| 2^-24, into the result as a relative error of that size"""
    zm = z.max(-1, keepdim=True).values
    p = torch.softmax(z, -1)
    return p, p * (1.0 + (z - zm).abs())


def softmax_logits(rows, n):
    x = normal((rows, n), 480 + rows + n, 2.0)
    x[rows // 2, n // 3] += 40.0                      # one row nearly one-hot
    return x


def softmax_rows(x, scale):
    return _softmax(t64(x) * scale)


def softmax_rows_f32(x, scale):
    z = x.float() * _t32(scale)
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


# (batch, T, L, mask_spec, scale): streams of two views; twin views from view 2 on; plain block-causal with a last view of 4 tokens;
# no mask; one token; one view that is not full
MASK_CASES = [(2, 96, 16, -2, 1.0), (1, 64, 16, 2, 1.0), (2, 100, 48, -1, 0.125), (1, 65, 0, -1, 1.0), (1, 1, 1, -1, 1.0), (1, 63, 64, -1, 1.0)]
MASKED_SCORE = -1e4                                   # the reference's w m - 1e4 (1 - m), branching_attention.py:11


def visible(T, L, spec, shift=0):
    """[T][T] bool: may query token q see key token k?  Views of L tokens (L = 0: no mask).  spec <= -2: streams of Sv = -spec views, the
    first stream block-causal over its own views, a later stream sees the first stream's earlier views (view index inside the stream) and
    its own view; spec >= 0: views from ``spec`` on are twins, each sees the views below ``spec`` and itself; spec = -1: block-causal.
    ``shift``: the mistake of a query view off by that many"""
    if L == 0:
        return torch.ones((T, T), dtype=torch.bool)
    v = torch.arange(T) // L
    q, k = v[:, None] + shift, v[None, :]
    if spec <= -2:
        Sv = -spec
        qs, qi, ks, ki = q // Sv, q % Sv, k // Sv, k % Sv
        return torch.where(qs == 0, (ks == 0) & (ki <= qi), ((ks == 0) & (ki < qi)) | (k == q))
    Vc = spec if spec >= 0 else 1 << 30
    return (k == q) | (k.clamp(max=Vc) < q.clamp(max=Vc))


def mask_inputs(batch, T, L, spec):
    """scores of std 3 (every row's visible maximum is far above -9000, so exp(-1e4 - max) is 0 in float32 and in float64) and dp"""
    return normal((batch, T, T), 500 + T + L, 3.0), normal((batch, T, T), 501 + T + L)


def softmax_mask(s, T, L, spec, scale, shift=0):
    """softmax over keys of (s scale) m - 1e4 (1 - m): a masked entry is exactly 0 (magnitude 0: the kernel must give 0)"""
    vis = visible(T, L, spec, shift)
    return _softmax(torch.where(vis, t64(s) * scale, torch.full((), MASKED_SCORE, dtype=F64)))


def softmax_mask_f32(s, T, L, spec, scale):
    z = torch.where(visible(T, L, spec), s.float() * _t32(scale), _t32(MASKED_SCORE))
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_mask_bwd(p, dp, T, L, spec, scale):
    """ds = scale p (dp - sum_j p_j dp_j), 0 where masked (p is 0 there)"""
    p, dp = t64(p), t64(dp)
    vis = visible(T, L, spec)
    s, sa = (p * dp).sum(-1, keepdim=True), (p * dp.abs()).sum(-1, keepdim=True)
    zero = torch.zeros((), dtype=F64)
    return torch.where(vis, scale * p * (dp - s), zero), torch.where(vis, abs(scale) * p * (dp.abs() + sa), zero)


def softmax_mask_bwd_f32(p, dp, T, L, spec, scale):
    p, dp = p.float(), dp.float()
    return torch.where(visible(T, L, spec), p * (dp - (p * dp).sum(-1, keepdim=True)) * _t32(scale), _t32(0.0))


# ------------------------------------------------------------------ softmax cross-entropy
CE_ROWS = [1, 5, 1027]
CE_V = [1, 63, 64, 65, 1026]
CE_SMOOTHING = [0.0, 0.1]
CE_SPREAD = (5, 1026)                                 # the case with logits spread over +/-60


def ce_inputs(rows, V, spread=False):
    """weights with exact zeros (every third row), targets in [0, V) with 0 and V - 1 planted"""
    logits = normal((rows, V), 520 + rows + V, 2.0)
    if spread:
        logits = torch.from_numpy(rng(521).uniform(-60.0, 60.0, size=(rows, V)).astype(np.float32))
    t = rng(522 + rows + V).integers(0, V, size=rows).astype(np.int32)
    t[0] = 0
    t[-1] = V - 1
    w = torch.from_numpy(rng(523 + rows).uniform(0.0, 1.0, size=rows).astype(np.float32))
    w[2::3] = 0.0
    return logits, torch.from_numpy(t), w


def softmax_ce(logits, target, w, eps):
    """y = onehot (1 - eps) + eps / V: loss = lse - sum_c y_c x_c, dlogits = (p - y) w
    -> ((loss, dlogits), (|max| + |log sum exp(x - max)| + sum_c y_c |x_c|, (p + onehot + eps / V) |w|)).
    A probability below float32's smallest normal number, 2^-126 (logits 87 below the row maximum: the +/-60 case), has no float32 value
    with 24 good bits and a kernel may flush it to 0: where the gradient's magnitude is not 0 it gets 2^-126 / 2^-24 added, so that the
    bound is c (2^-24 magnitude + 2^-126).  A row of weight 0 keeps magnitude 0: its gradient must be exactly 0"""
    x, w = t64(logits), t64(w)
    V = x.shape[-1]
    one = torch.zeros_like(x).scatter_(1, target.long().view(-1, 1), 1.0)
    y = one * (1.0 - eps) + eps / V
    mx = x.max(-1).values
    ls = torch.log(torch.exp(x - mx[:, None]).sum(-1))
    p = torch.softmax(x, -1)
    md = (p + one + eps / V) * w.abs()[:, None]
    return ((mx + ls) - (y * x).sum(-1), (p - y) * w[:, None]), (mx.abs() + ls.abs() + (y * x.abs()).sum(-1), torch.where(md > 0, md + F32_TINY / U, md))


def softmax_ce_f32(logits, target, w, eps):
    x, w = logits.float(), w.float()
    V = x.shape[-1]
    e32 = _t32(eps)
    mx = x.max(-1, keepdim=True).values
    ex = torch.exp(x - mx)
    s = ex.sum(-1, keepdim=True)
    lse = mx[:, 0] + torch.log(s[:, 0])
    xt = x.gather(1, target.long().view(-1, 1))[:, 0]
    uni = e32 / _t32(float(V))
    loss = lse - (1.0 - e32) * xt - uni * x.sum(-1) if eps != 0.0 else lse - xt
    one = torch.zeros_like(x).scatter_(1, target.long().view(-1, 1), 1.0)
    return loss, (ex / s - (one * (1.0 - e32) + uni)) * w[:, None]


def softmax_ce_without_uniform_term(logits, target, w, eps):
    """the mistake: the eps / V share of the smoothed target left out of loss and gradient"""
    x, w = t64(logits), t64(w)
    one = torch.zeros_like(x).scatter_(1, target.long().view(-1, 1), 1.0)
    return torch.logsumexp(x, -1) - (1.0 - eps) * (one * x).sum(-1), (torch.softmax(x, -1) - one * (1.0 - eps)) * w[:, None]


# ------------------------------------------------------------------ AdamWeightDecay
ADAMW_SIZES = [1, 1027, 8192 * 256 + 3]               # the last: past the capped grid (second lap), on the device
ADAMW_HYPER = (1e-3 * 0.05, 2e-3, 0.9, 0.999, 1e-8)   # lr_decay = lr x weight_decay, lr_adam = the bias-corrected lr, beta1, beta2, eps


def adamw_hyper():
    """the float32 values the kernel receives, as Python floats"""
    return tuple(f32(h) for h in ADAMW_HYPER)


def adamw_inputs(n, device='cpu'):
    """(param, grad, m, v >= 0); elements with g = 0, with m = 0, with v = 0 and one with all three"""
    if str(device) == 'cpu':
        p, g, m, v = normal((n,), 540), normal((n,), 541), normal((n,), 542, 0.1), normal((n,), 543, 0.01).abs()
    else:
        gen = torch.Generator(device=device).manual_seed(540)
        p, g, m, v = (torch.randn((n,), generator=gen, device=device) * sc for sc in (1.0, 1.0, 0.1, 0.01))
        v = v.abs()
    g[::7] = 0.0
    m[::11] = 0.0
    v[::13] = 0.0
    return p, g, m, v


def adamw(p, g, m, v, lr_decay, lr_adam, b1, b2, eps, nodecay=None):
    """w -= lr_decay w (not where ``nodecay``), m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, w -= lr_adam m / (sqrt(v) + eps), with
    1 - beta formed in float32 from the float32 betas (exact for beta in [0.5, 1)) -> ((w, m, v), magnitudes)"""
    p, g, m, v = t64(p), t64(g), t64(m), t64(v)
    ob1, ob2 = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    ld = lr_decay if nodecay is None else (~nodecay.to(p.device)).to(F64) * lr_decay
    m1, ma = b1 * m + ob1 * g, b1 * m.abs() + ob1 * g.abs()
    v1 = b2 * v + ob2 * g * g
    den = torch.sqrt(v1) + eps
    return (p - ld * p - lr_adam * m1 / den, m1, v1), (p.abs() + ld * p.abs() + lr_adam * ma / den, ma, v1)


def adamw_f32(p, g, m, v, lr_decay, lr_adam, b1, b2, eps, nodecay=None):
    p, g, m, v = p.float(), g.float(), m.float(), v.float()
    ld = _t32(lr_decay) if nodecay is None else torch.where(nodecay, _t32(0.0), _t32(lr_decay))
    m1 = _t32(b1) * m + (1.0 - _t32(b1)) * g
    v1 = _t32(b2) * v + ((1.0 - _t32(b2)) * g) * g
    return (p - ld * p) - (_t32(lr_adam) * m1) / (torch.sqrt(v1) + _t32(eps)), m1, v1


ADAMW_FLAT_N = 4096
ADAMW_FLAT_RANGES = {                                 # sorted, disjoint [start, end) element ranges that skip the decay, on multiples of 4
    'none': [],
    'one_at_0': [(0, 64)],
    'two_adjacent': [(128, 256), (256, 300)],
    'last_ends_at_n': [(64, 128), (4000, ADAMW_FLAT_N)],
    '256_ranges': [(16 * k + 4, 16 * k + 12) for k in range(256)],
}


def nodecay_mask(n, ranges):
    mask = torch.zeros(n, dtype=torch.bool)
    for a, b in ranges:
        mask[a:b] = True
    return mask


def segments(n, ranges):
    """the flat buffer cut into the tensors an update tensor by tensor walks: [(start, end, nodecay)]"""
    out, at = [], 0
    for a, b in ranges:
        if at < a:
            out.append((at, a, False))
        out.append((a, b, True))
        at = b
    if at < n:
        out.append((at, n, False))
    return out


# ------------------------------------------------------------------ tiny dense, K <= 16
DENSE_K_CASES = [(1, 1, 1), (1000, 7, 129), (300, 16, 256)]


def dense_k_inputs(rows, K, N):
    return normal((rows, K), 560 + K), normal((K, N), 561 + K + N, 0.5), normal((N,), 562 + N)


def dense_small_k(x, W, b, gelu_on):
    """x W [+ b], GELU on request.  Magnitude |x| |W| + |b|, for the GELU's output as well: |gelu'| <= 1.13 carries the sum's error over
    at most as it stands and |gelu(a)| <= |a| bounds the GELU's own rounding by the same figure"""
    a, ma = t64(x) @ t64(W), t64(x).abs() @ t64(W).abs()
    if b is not None:
        a, ma = a + t64(b), ma + t64(b).abs()
    return (gelu(a)[0] if gelu_on else a), ma


def dense_small_k_f32(x, W, b, gelu_on):
    """the kernel's running sum over k, then the bias"""
    x, W = x.float(), W.float()
    a = torch.zeros((x.shape[0], W.shape[1]), dtype=F32)
    for k in range(x.shape[1]):
        a = a + x[:, k:k + 1] * W[k:k + 1]
    if b is not None:
        a = a + b.float()
    return gelu_f32(a) if gelu_on else a
