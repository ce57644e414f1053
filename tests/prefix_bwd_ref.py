"""Shared by tests/test_prefix_bwd_ref_host.py and tests/test_hip_prefix_bwd.py: the float64 reference of the prefix-cache attention's
backward over the query views (csrc/attention_prefix_bwd.hip), the fp32 restatement of the kernel's two passes in its tile order, and the
inputs and cases.  No device is needed to import or to run this.

For query view (b, n) of length c and head h, with K = [Kp[:c L]; K_own], V likewise (thirds of the fused c_attn output: V, Q, K):
    S = Q K^T (un-scaled),  P = softmax(S),  O = P V,  D = rowsum(dO * O),  dP = dO V^T,  dS = P * (dP - D)
    dQ = dS K,   dK_own = dS[:, own]^T Q,   dV_own = P[:, own]^T dO
and the output rows are (dV_own | dQ | dK_own), the c_attn column order.  The cache is a constant.

Magnitudes.  Every reference output comes with a magnitude: the same expression with every summand replaced by its absolute value, so
that ``c * 2^-24 * magnitude`` bounds what fp32 arithmetic in any order may do to it.  P carries the error of its score and of its
log-sum-exp: |P| = P (1 + Sa + E) with Sa = |Q| |K|^T and E = rowsum(P * Sa) (tests/attention_kernels_ref.py uses the same form).  Then
|O| = |P| |V|,  |D| = rowsum(|dO| |O|),  |dP| = |dO| |V|^T,  |dS| = |P| (|dP| + |D|),  |dQ| = |dS| |K|,  |dK| = |dS|^T |Q|,  |dV| = |P|^T |dO|."""
import numpy as np
import torch

L = 64
DH = 64
UNIT = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
LOG2E = 1.4426950408889634

# the GPU test's constants, one per output: tests/test_prefix_bwd_ref_host.py::test_calibration derives each (4 x the restatement's worst
# error of that output in units of 2^-24 x magnitude over all cases, rounded up to a power of two) and asserts that these lines say the
# same.  The magnitudes of dQ and dK carry the factor 1 + Sa + E of |P| twice over (through |dS|), so their errors are small fractions
# of a unit: one constant for all three would leave their check a few hundred times of slack.
OUTPUTS = ('dv', 'dq', 'dk')                                    # the thirds of dqkv, in column order
C_BOUND = dict(dv=8.0,          # restatement's worst: 1.13 units (case 'peaked', fp32 storage)
               dq=0.0625,       # 0.0107 units (case 'mixed_lengths', fp32 storage)
               dk=0.125)        # 0.0202 units (case 'mixed_lengths', fp32 storage)

# wrong kernels the bounds must reject: four gross ones, and a subtle one (D from an O rounded to bf16, what taking the bf16 arm's forward
# output instead of recomputing O would give) that only the bounds of dQ and dK can see
MUTANTS = ('no_D', 'dk_from_prefix', 'p_without_lse', 'columns_swapped', 'D_from_bf16_O')


def rand(shape, seed, scale):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


# (name, (B, H, C, N), lengths [B][N] or None (all C), kind): the smallest shapes at which the kernel can still go wrong.  q and k are
# N(0, 0.35^2), so the un-scaled scores have unit spread; 'peaked': N(0, 0.7^2), score spread 4: the running maximum moves at almost
# every 32-key step of pass 1
CASES = [
    ('smallest', (1, 1, 1, 1), None, 'normal'),
    ('mixed_lengths', (2, 2, 3, 3), [[0, 3, 1], [2, 2, 3]], 'normal'),
    ('peaked', (2, 2, 3, 3), [[0, 3, 1], [2, 2, 3]], 'peaked'),
    ('d768', (1, 12, 2, 1), None, 'normal'),
    ('scene_lengths', (2, 2, 4, 4), [[2, 2, 2, 2], [2, 2, 2, 2]], 'normal'),
]
BY_NAME = {c[0]: c for c in CASES}
STORAGE = ('f32', 'bf16')


def case_id(case):
    return case[0]


def lengths_of(case):
    _, (B, H, C, N), lens, _ = case
    return np.full((B, N), C, dtype=np.int32) if lens is None else np.asarray(lens, dtype=np.int32).reshape(B, N)


def inputs(case, storage='f32'):
    """(ctx [B, C*L, 3d], qkv [B*N*L, 3d], dout [B*N*L, d]) as STORED: fp32, or rounded to bf16 (``storage='bf16'``; dout stays fp32)"""
    _, (B, H, C, N), _, kind = case
    d = H * DH
    s = 0.7 if kind == 'peaked' else 0.35
    seed = 1000 * B + 100 * H + 10 * C + N + (5000 if kind == 'peaked' else 0)
    ctx = rand((B, C * L, 3 * d), seed + 1, s)
    qkv = rand((B * N * L, 3 * d), seed + 2, s)
    dout = rand((B * N * L, d), seed + 3, 1.0)
    if storage == 'bf16':
        ctx, qkv = ctx.to(torch.bfloat16), qkv.to(torch.bfloat16)
    return ctx, qkv, dout


def _view_operands(ctx, qkv, dout, b, n, h, c, N, dtype):
    """(Q, K_all, V_all, dO) of view (b, n), head h with c prefix views: [L,64], [(c+1)L,64] x 2, [L,64]"""
    d = ctx.shape[-1] // 3
    hs = slice(h * DH, (h + 1) * DH)
    rows = slice((b * N + n) * L, (b * N + n + 1) * L)
    third = lambda x, i: x[..., i * d:(i + 1) * d][..., hs].to(dtype)
    q, k, v = third(qkv[rows], 1), third(qkv[rows], 2), third(qkv[rows], 0)
    kp, vp = third(ctx[b, :c * L], 2), third(ctx[b, :c * L], 0)
    return q, torch.cat([kp, k], 0), torch.cat([vp, v], 0), dout[rows][:, hs].to(dtype)


def reference(case, storage='f32', mut=None, lengths=None):
    """float64 reference of the values as stored -> (dqkv [B*N*L, 3d], magnitude [B*N*L, 3d]), columns (dV | dQ | dK).  ``mut``: one of
    MUTANTS, a wrong kernel that the bound must reject (tests/test_prefix_bwd_ref_host.py)."""
    _, (B, H, C, N), _, _ = case
    d = H * DH
    lens = lengths_of(case) if lengths is None else np.asarray(lengths).reshape(B, N)
    ctx, qkv, dout = inputs(case, storage)
    out = torch.zeros((B * N * L, 3 * d), dtype=F64)
    mag = torch.zeros_like(out)
    order = (1, 2, 0) if mut == 'columns_swapped' else (0, 1, 2)        # thirds that receive (dV, dQ, dK)
    for b in range(B):
        for n in range(N):
            c = int(lens[b, n])
            rows = slice((b * N + n) * L, (b * N + n + 1) * L)
            for h in range(H):
                q, k, v, do = _view_operands(ctx, qkv, dout, b, n, h, c, N, F64)
                S = q @ k.T
                Sa = q.abs() @ k.abs().T
                if mut == 'p_without_lse':
                    P = torch.exp(S - S.amax(1, keepdim=True))
                else:
                    P = torch.softmax(S, 1)
                Pm = P * (1.0 + Sa + (P * Sa).sum(1, keepdim=True))
                O, Om = P @ v, Pm @ v.abs()
                D, Dm = (do * O).sum(1, keepdim=True), (do.abs() * Om).sum(1, keepdim=True)
                if mut == 'no_D':
                    D = torch.zeros_like(D)
                if mut == 'D_from_bf16_O':
                    D = (do * O.to(torch.bfloat16).double()).sum(1, keepdim=True)
                dP, dPm = do @ v.T, do.abs() @ v.abs().T
                dS, dSm = P * (dP - D), Pm * (dPm + Dm)
                own = slice(c * L, (c + 1) * L)
                kown = slice(0, L) if (mut == 'dk_from_prefix' and c > 0) else own
                vals = (P[:, own].T @ do, dS @ k, dS[:, kown].T @ q)
                mags = (Pm[:, own].T @ do.abs(), dSm @ k.abs(), dSm[:, own].T @ q.abs())
                for third, x, m in zip(order, vals, mags):
                    cols = slice(third * d + h * DH, third * d + (h + 1) * DH)
                    out[rows, cols], mag[rows, cols] = x, m
    return out, mag


# ------------------------------------------------------------------ the kernel's arithmetic, restated in fp32
def _mm(a, bt):
    """a [m,64] . bt[n,64]^T in fp32, the contraction in the kernel's order: one 32x32x2 product adds features (8 g + e, 8 g + 4 + e), g and
    e ascending — 32 updates of two products each.  Elementwise torch ops: the same bits on every host."""
    acc = torch.zeros((a.shape[0], bt.shape[0]), dtype=F32)
    for g in range(8):
        for e in range(4):
            f0, f1 = 8 * g + e, 8 * g + 4 + e
            acc = acc + (a[:, f0:f0 + 1] * bt[:, f0][None] + a[:, f1:f1 + 1] * bt[:, f1][None])
    return acc


def _mm_keys(p, x):
    """p [m, 32 keys] . x [32 keys, 64] in fp32, keys in pairs (8 j + e, 8 j + 4 + e), j and e ascending: the accumulation over a 32-key step"""
    acc = torch.zeros((p.shape[0], x.shape[1]), dtype=F32)
    for j in range(4):
        for e in range(4):
            k0, k1 = 8 * j + e, 8 * j + 4 + e
            acc = acc + (p[:, k0:k0 + 1] * x[k0][None] + p[:, k1:k1 + 1] * x[k1][None])
    return acc


def restatement(case, storage='f32'):
    """the kernel in fp32 torch on the CPU: operands widened to fp32, 32-key steps in the kernel's order, pass 1 (running max / sum with a
    rescale per step, O, then lse = m + log l and D = (dO . O~) / l), pass 2 (P = exp2((S - lse) log2 e), dS, dQ), own tile per 32-query
    half.  -> dqkv fp32 [B*N*L, 3d]"""
    _, (B, H, C, N), _, _ = case
    d = H * DH
    lens = lengths_of(case)
    ctx, qkv, dout = inputs(case, storage)
    out = torch.zeros((B * N * L, 3 * d), dtype=F32)
    log2e = torch.tensor(LOG2E, dtype=F32)
    for b in range(B):
        for n in range(N):
            c = int(lens[b, n])
            rows = slice((b * N + n) * L, (b * N + n + 1) * L)
            for h in range(H):
                q, k, v, do = _view_operands(ctx, qkv, dout, b, n, h, c, N, F32)
                steps = [(k[i:i + 32], v[i:i + 32]) for i in range(0, (c + 1) * L, 32)]
                m = torch.full((L, 1), -float('inf'), dtype=F32)
                l = torch.zeros((L, 1), dtype=F32)
                o = torch.zeros((L, DH), dtype=F32)
                for ks, vs in steps:                                             # pass 1
                    s = _mm(q, ks)
                    m_new = torch.maximum(m, s.amax(1, keepdim=True))
                    alpha = torch.exp2((m - m_new) * log2e)
                    p = torch.exp2((s - m_new) * log2e)
                    l = l * alpha + p.sum(1, keepdim=True)
                    o = o * alpha + _mm_keys(p, vs)
                    m = m_new
                D = (do * o).sum(1, keepdim=True) / l
                lse = m + torch.log(l)
                dq = torch.zeros((L, DH), dtype=F32)
                for ks, vs in steps:                                             # pass 2
                    p = torch.exp2((_mm(q, ks) - lse) * log2e)
                    ds = p * (_mm(do, vs) - D)
                    dq = dq + _mm_keys(ds, ks)
                ko, vo = k[c * L:], v[c * L:]
                dk = torch.zeros((L, DH), dtype=F32)
                dv = torch.zeros((L, DH), dtype=F32)
                for t2 in range(2):                                              # own tile: the two 32-query halves
                    qs = slice(32 * t2, 32 * t2 + 32)
                    p = torch.exp2((_mm(q[qs], ko) - lse[qs]) * log2e)           # [32 queries, 64 keys]
                    ds = p * (_mm(do[qs], vo) - D[qs])
                    dv = dv + _mm_keys(p.T.contiguous(), do[qs])
                    dk = dk + _mm_keys(ds.T.contiguous(), q[qs])
                for third, x in zip((0, 1, 2), (dv, dq, dk)):
                    out[rows, third * d + h * DH:third * d + (h + 1) * DH] = x
    return out


def worst_ratio(got, want, mag):
    """max |got - want| / (2^-24 magnitude) over all elements"""
    return float(((got.double() - want).abs() / (UNIT * mag)).max())


def worst_ratios(got, want, mag):
    """{'dv', 'dq', 'dk'} -> worst_ratio over that third of the columns"""
    d = want.shape[1] // 3
    return {t: worst_ratio(got[:, i * d:(i + 1) * d], want[:, i * d:(i + 1) * d], mag[:, i * d:(i + 1) * d]) for i, t in enumerate(OUTPUTS)}
