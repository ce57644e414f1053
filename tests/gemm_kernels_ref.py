"""Test infrastructure of the per-kernel tests of the bf16 GEMM family (tests/test_hip_gemm_kernels.py on the GPU,
tests/test_gemm_kernels_ref_host.py on the CPU), built like tests/transformer_kernels_ref.py and on its helpers: the forward GEMM
vf_gemm_bf16 with every epilogue form of its three kernels (the staged 128-tile kernel, the direct 128-tile kernel, the 256-tile
kernel with and without tail tiles), the weight-gradient GEMM vf_gemm_tn_bf16, the slab fold vf_sum_slabs_f32 and the bf16 packings.

For every operation: a float64 restatement written from include/vf_hip.h and the docstring of ops.igemm, returning ``(value, magnitude)``.
The operands of the matrix product are the bf16 roundings (to nearest even) of x and W — x as it is stored when it arrives as bf16 — and a
product of two bf16 values is exact in float32, so only the order of the float32 sums separates a correct kernel from the reference: the
magnitude is the same expression with every summand replaced by its absolute value.  An epilogue function adds its own term to the
magnitude, in units of 2^-24 (``FN_TERM``): every GELU and GELU derivative of the bf16 arm evaluates erf by Abramowitz & Stegun 7.1.26,
whose absolute error csrc/vf_common.h states as 1.5e-7 (X.ERF_AS_ERR), scaled by what multiplies the erf — as X.gelu_bwd_bf16_bound does.
``*_f32`` functions restate the KERNEL's order on torch-CPU float32: 16 k per matrix instruction inside 64-deep chunks along k in order
(64-row chunks, then the slab fold, for the weight gradient), then the epilogue in float32.  They are used for calibration only: the host
test measures their distance from float64 on the very inputs of the GPU test, and the GPU test's constants come from that measurement,
never from the kernel.

A bf16 output is judged by the INTERVAL RULE: with b the float32 bound c x 2^-24 x magnitude, bf16_rne(want - b) <= got <= bf16_rne(want + b).
A correct kernel rounds a float32 value inside [want - b, want + b] to nearest even, and rounding is monotonic, so it cannot leave that
interval; truncation and a second rounding do.  No element is excluded.

Input generators and case tables live here so that both files see the same tensors.  Nothing is imported from viewformer_amd except the
host evaluation of the dropout hash (_hash): the mask is an integer definition, restated there once for every host-side check."""
import numpy as np
import torch

import training_kernels_ref as R
import transformer_kernels_ref as X
from training_kernels_ref import U, F64, t64, rng, normal  # noqa: F401  (one definition of each, shared)
from viewformer_amd import _hash

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -1.5 * 2.0 ** 100                          # exact in bf16 and float32; no result of any case comes near it
BAD_ARG, UNSUPPORTED = -1, -2
FN_TERM = X.ERF_AS_ERR / U                            # the stated |erf error| in units of 2^-24: 2.52


# ------------------------------------------------------------------ bf16
def bf16_rne(v):
    """the bf16 value (round to nearest even) of float64 or float32 values, as float64.  A float64 passes through float32 first: for the
    interval rule that is the right order (a kernel's float32 value v >= want - b is >= float32(want - b), and bf16 rounding is monotonic)"""
    return torch.as_tensor(v).to(F32).to(BF16).to(F64)


def bf16_trunc(v):
    """the mistake: the upper 16 bits of the float32 pattern"""
    bits = torch.as_tensor(v).to(F32).contiguous().view(torch.int32) & -65536
    return bits.view(F32).to(F64)


def as16(x):
    """the GEMM operand: a bf16 tensor as it is stored, a float32 tensor rounded to nearest even"""
    return x.to(F64) if x.dtype == BF16 else bf16_rne(x)


def interval_violations(got16, want, bound):
    """the interval rule: number of elements outside [bf16_rne(want - bound), bf16_rne(want + bound)]; a NaN is outside"""
    got, want, bound = t64(got16.float() if got16.dtype == BF16 else got16), t64(want), t64(bound)
    if got.shape != want.shape:
        return max(got.numel(), want.numel(), 1)
    return int((~((got >= bf16_rne(want - bound)) & (got <= bf16_rne(want + bound)))).sum())


def bound(mag, c):
    return c * U * t64(mag)


# ------------------------------------------------------------------ inputs
def ints(shape, seed, hi=8):
    """float32 integers in [-hi, hi]"""
    return torch.from_numpy(rng(seed).integers(-hi, hi + 1, size=shape).astype(np.float32))


def eighths(shape, seed):
    """float32 multiples of 1/8 in (-8, 8) (exact in bf16) with exact zeros and -0.0.  Times an integer of at most 8, summed over at most
    640 terms: below 2^16 on a grid of 2^-3, exact in float32 in any order"""
    g = rng(seed)
    a = (g.integers(-63, 64, size=shape).astype(np.float32) / 8.0).reshape(-1)
    k = max(1, a.size // 16)
    a[g.integers(0, a.size, size=k)] = 0.0
    a[g.integers(0, a.size, size=k)] = -0.0
    return torch.from_numpy(a.reshape(shape))


def pow2_table(shape, seed):
    """bf16 values in {0, +-1/4, +-1/2, +-1, +-2}: a saved-derivative table whose product with a dyadic sum is exact"""
    v = torch.tensor([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=F32)
    return v[torch.from_numpy(rng(seed).integers(0, 9, size=shape))].to(BF16)


def permutation(n, seed):
    return torch.from_numpy(rng(seed).permutation(n))


def selector(n, seed):
    """x [n][n] with a single 1 per row, at column pi(m): x @ W = W[pi], x^T @ dy = dy[pi^-1] -> (x, pi)"""
    pi = permutation(n, seed)
    x = torch.zeros((n, n), dtype=F32)
    x[torch.arange(n), pi] = 1.0
    return x, pi


def u_input(M, N, seed):
    """the saved pre-activation: 1.5 N(0, 1), its first elements replaced by X.gelu_sweep ([-12, 12] in steps of 2^-6: GELU's negative tail)"""
    u = normal((M, N), seed, 1.5).reshape(-1)
    sw = X.gelu_sweep()
    k = min(u.numel(), sw.numel())
    u[:k] = sw[(torch.arange(k) * 1021 + 700) % sw.numel()]
    return u.view(M, N)


def forward_inputs(M, K, N, cls, seed=0, saved=True):
    """cls 'normal': x ~ N(0, 1), W ~ 0.05 N(0, 1), bias and residual ~ N(0, 1), u as u_input, the derivative table bf16 N(0.5, 0.4);
    cls 'dyadic': integers |x| <= 8, multiples of 1/8 in W, bias and residual, a table of powers of two: every partial sum is exact.
    ``saved`` = False leaves out u and the table (the tail-tile cases have no form that reads them)"""
    s = 7000 + 131 * (M % 1009) + 17 * K + N + seed
    if cls == 'dyadic':
        inp = dict(x=ints((M, K), s), W=eighths((K, N), s + 1), bias=eighths((N,), s + 2), res=eighths((M, N), s + 3))
    else:
        inp = dict(x=normal((M, K), s), W=normal((K, N), s + 1, 0.05), bias=normal((N,), s + 2), res=normal((M, N), s + 3))
    if saved:
        inp.update(u=u_input(M, N, s + 4), g16=pow2_table((M, N), s + 5) if cls == 'dyadic' else normal((M, N), s + 5, 0.4, 0.5).to(BF16))
    return inp


def tn_inputs(M, K, N, cls, seed=0):
    """x16 bf16 [M][K], dy float32 [M][N]: 'normal' N(0, 1) and 0.1 N(0, 1); 'dyadic' integers and multiples of 1/8"""
    s = 9000 + 131 * M + 17 * K + N + seed
    if cls == 'dyadic':
        return ints((M, K), s).to(BF16), eighths((M, N), s + 1)
    return normal((M, K), s).to(BF16), normal((M, N), s + 1, 0.1)


# ------------------------------------------------------------------ forward GEMM: float64
def gemm(x, W, bias=None):
    """pre = bf16_rne(x) @ bf16_rne(W) + bias, magnitude |x16| @ |W16| + |bias|"""
    x16, W16 = as16(x), as16(W)
    pre, mag = x16 @ W16, x16.abs() @ W16.abs()
    if bias is not None:
        pre, mag = pre + t64(bias), mag + t64(bias).abs()
    return pre, mag


def gelu_grad(u):
    """gelu'(u) = Phi(u) + u phi(u) and the same with absolute values"""
    one = torch.ones_like(t64(u))
    return X.gelu_bwd(u, one)


def drop_keep(rows, N, rate, seed, site, row0):
    """keep(m + row0, n) of the mask train_ops.dropout_add draws with cols = N, for the row indices ``rows`` -> bool [len(rows)][N]"""
    m = (np.asarray(rows, dtype=np.uint64) + np.uint64(row0))[:, None]
    n = np.arange(N, dtype=np.uint64)[None, :]
    g, sub = _hash.elem_group(np.broadcast_to(m, (m.shape[0], N)), n, N)
    if g.size <= 1 << 17:
        return torch.from_numpy(np.ascontiguousarray(_hash.dropout_keep(seed, site, g, sub, X.f32(rate))))
    # _hash.dropout_keep looks the key of every element's upper index half up one by one; every group index here is below 2^32, so the key
    # is the one of upper half 0 and the same definition is evaluated on whole arrays (the host test holds the two against each other)
    assert int(g.max()) < 2 ** 32
    w = _hash.lowbias32(g ^ np.uint64(int(_hash.dropout_hash(seed, site, [0])[0]))).astype(np.uint64)
    sh = sub.astype(np.uint64) * np.uint64(8)
    rot = ((w << sh) | (w >> (np.uint64(32) - sh))) & np.uint64(0xFFFFFFFF)
    return torch.from_numpy(np.ascontiguousarray(rot >= np.uint64(int(X.f32(rate) * 4294967296.0))))


# form -> what the launch carries.  'res' and 'gelu_res' exist with a float32 output only, 'dual_grad', 'gelu_bwd*' with a bf16 output only
FORMS = {
    'none': dict(),
    'bias': dict(bias=True),
    'res': dict(bias=True, res=True),
    'gelu': dict(bias=True, epi='gelu'),
    'gelu_res': dict(bias=True, epi='gelu', res=True),
    'dual': dict(bias=True, epi='dual'),
    'dual_grad': dict(bias=True, epi='dual', gelu_grad=True),
    'gelu_bwd': dict(epi='gelu_bwd'),                                  # u float32 behind `res`
    'gelu_bwd16': dict(epi='gelu_bwd', res16=True),                    # u bf16
    'gelu_bwd16_grad': dict(epi='gelu_bwd', res16=True, gelu_grad=True),   # the saved derivative behind `res`
    'drop': dict(bias=True, drop=True),
    'drop_res': dict(bias=True, drop=True, res=True),
}
# which function class (the suffix of the constant's name) judges an output of a form
FN_CLASS = {'gelu': 'gelu', 'gelu_res': 'gelu', 'dual_grad': 'gelu_grad', 'gelu_bwd': 'gelu_bwd', 'gelu_bwd16': 'gelu_bwd',
            'drop': 'drop', 'drop_res': 'drop'}


def fn_class(form, name='out'):
    if form in ('dual', 'dual_grad') and name == 'aux':
        return 'gelu'
    return FN_CLASS.get(form, '')


def epilogue(form, pre, mag, res=None, u=None, g16=None, keep=None, rate=0.0):
    """the outputs of a form from the float64 pre-activation (bias included) and its magnitude -> {'out': (want, mag)[, 'aux': ...]}:
      out = epi(pre) + res                       epi = identity or GELU; the residual joins after the function
      dual: out = pre, aux = gelu(pre)           aux from the unrounded pre; dual_grad: out = gelu'(pre) instead
      gelu_bwd: out = pre gelu'(u)               u as it is stored (float32 or bf16); gelu_bwd16_grad: out = pre g16, g16 the saved derivative
      drop: out = res + keep pre / (1 - rate)    a dropped element is exactly res (magnitude |res|, 0 without a residual)
    Magnitudes: a GELU output is judged against the magnitude of its argument (|gelu'| <= 1.13, |gelu(a)| <= |a|) plus the erf
    approximation's 0.5 |pre| FN_TERM; gelu'(pre) against that of pre (|gelu''| <= 0.8) plus its own |Phi| + |u| phi and 0.5 FN_TERM;
    pre gelu'(u) against mag(pre) (|Phi(u)| + |u| phi(u)) plus |pre| FN_TERM"""
    f = FORMS[form]
    out = {}
    if f.get('epi') == 'gelu':
        w, m = X.gelu(pre)[0], mag + 0.5 * pre.abs() * FN_TERM
    elif f.get('epi') == 'dual':
        out['aux'] = (X.gelu(pre)[0], mag + 0.5 * pre.abs() * FN_TERM)
        if f.get('gelu_grad'):
            d, dm = gelu_grad(pre)
            w, m = d, mag + dm + 0.5 * FN_TERM
        else:
            w, m = pre, mag
    elif f.get('epi') == 'gelu_bwd':
        if f.get('gelu_grad'):
            w, m = pre * t64(g16.float()), mag * t64(g16.float()).abs()
        else:
            d, dm = gelu_grad(u.float())
            w, m = pre * d, mag * dm + pre.abs() * FN_TERM
    elif f.get('drop'):
        scale = 1.0 / (1.0 - X.f32(rate))
        zero = torch.zeros((), dtype=F64)
        w, m = torch.where(keep, pre * scale, zero), torch.where(keep, mag * scale, zero)
    else:
        w, m = pre, mag
    if f.get('res'):
        w, m = w + t64(res), m + t64(res).abs()
    out['out'] = (w, m)
    return out


# ------------------------------------------------------------------ forward GEMM: the kernel's order on float32
MFMA_K, CHUNK_K = 16, 64


def gemm_f32(x, W, bias=None, k_range=None, lost=None):
    """one float32 accumulator per element, 16 k per step in ascending order (the 64-deep chunks follow each other, so the chunk boundary
    adds nothing to the order): a step's 16 exact products are summed without rounding (float64 holds them) and join the accumulator with
    one float32 rounding; the bias is added last.  ``lost`` = (m0, m1, n0, n1, k0): the mistake of one 16-deep step left out in a tile.
    (Measured afterwards, profiles/gemm_kernels_parity.txt 2: the instruction itself rounds after every 8 k.  The step stays the instruction's
    depth: the calibration states an order that is valid, not the hardware's, and the factor 4 on its figure is what covers the difference)"""
    x16, W16 = as16(x).to(F32), as16(W).to(F32)
    k0, k1 = (0, x16.shape[1]) if k_range is None else k_range
    acc = torch.zeros((x16.shape[0], W16.shape[1]), dtype=F32)
    for k in range(k0, k1, MFMA_K):
        step = x16[:, k:k + MFMA_K].to(F64) @ W16[k:k + MFMA_K].to(F64)          # exact: no BLAS's order of the 16 enters the figure
        if lost is not None and lost[4] == k:
            step[lost[0]:lost[1], lost[2]:lost[3]] = 0.0
        acc = (acc.to(F64) + step).to(F32)
    return acc + bias.to(F32) if bias is not None else acc


def _t32(v):
    return torch.tensor(v, dtype=F32)


def _erf_pieces_f32(v):
    """1 + erf(v / sqrt 2) and exp(-v^2 / 2) as the bf16 arm forms them: Abramowitz & Stegun 7.1.26 on an exp2"""
    z = v.abs() * _t32(X.RSQRT2)
    t = 1.0 / (_t32(0.3275911) * z + 1.0)
    p = _t32(1.061405429) * t + _t32(-1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + _t32(c)
    e = torch.exp2(_t32(-1.4426950408889634) * (z * z))
    return 1.0 + torch.copysign(1.0 - (p * t) * e, v), e


def gelu_fast_f32(v):
    return _t32(0.5) * v * _erf_pieces_f32(v)[0]


def gelu_grad_fast_f32(v):
    one_plus, e = _erf_pieces_f32(v)
    return v * (_t32(X.RSQRT2PI) * e) + _t32(0.5) * one_plus


def epilogue_f32(form, acc, res=None, u=None, g16=None, keep=None, rate=0.0):
    """the epilogue on the float32 accumulator (bias included) -> {'out': float32[, 'aux': float32]}: the values before an output's bf16 rounding"""
    f = FORMS[form]
    out = {}
    if f.get('epi') == 'gelu':
        v = gelu_fast_f32(acc)
    elif f.get('epi') == 'dual':
        out['aux'] = gelu_fast_f32(acc)
        v = gelu_grad_fast_f32(acc) if f.get('gelu_grad') else acc
    elif f.get('epi') == 'gelu_bwd':
        v = acc * (g16.to(F32) if f.get('gelu_grad') else gelu_grad_fast_f32(u.to(F32)))
    elif f.get('drop'):
        v = torch.where(keep, acc * (_t32(1.0) / (_t32(1.0) - _t32(rate))), _t32(0.0))
    else:
        v = acc
    if f.get('res'):
        v = v + res.to(F32)
    out['out'] = v
    return out


def _operands(form, inp, rows, drop):
    """the epilogue's operands of a form from an input set, restricted to ``rows``: u as bf16 where the form saves it so, the keep mask of
    ``drop`` = (rate, row0) for the global row indices"""
    f = FORMS[form]
    M, N = inp['x'].shape[0], inp['W'].shape[1]
    rows = torch.arange(M) if rows is None else rows
    kw = {}
    if f.get('res'):
        kw['res'] = inp['res'][rows]
    if f.get('epi') == 'gelu_bwd' and f.get('gelu_grad'):
        kw['g16'] = inp['g16'][rows]
    elif f.get('epi') == 'gelu_bwd':
        kw['u'] = inp['u'][rows].to(BF16) if f.get('res16') else inp['u'][rows]
    if f.get('drop'):
        kw.update(keep=drop_keep(rows.numpy(), N, drop[0], DROP_SEED, DROP_SITE, drop[1]), rate=drop[0])
    return kw


def wants(form, inp, pre0, mag0, rows=None, drop=None):
    """{'out': (want, magnitude)[, 'aux': ...]} of a form from the float64 product without its bias (shared by the forms of a shape)"""
    if FORMS[form].get('bias'):
        pre0, mag0 = pre0 + t64(inp['bias']), mag0 + t64(inp['bias']).abs()
    return epilogue(form, pre0, mag0, **_operands(form, inp, rows, drop))


def restated(form, inp, acc0, rows=None, drop=None):
    """the same from the float32 accumulator of gemm_f32 without its bias: float32 values before an output's bf16 rounding"""
    if FORMS[form].get('bias'):
        acc0 = acc0 + inp['bias'].to(F32)
    return epilogue_f32(form, acc0, **_operands(form, inp, rows, drop))


# ------------------------------------------------------------------ the slab fold: exact class
def fold_f32(slabs, dst0=None, reverse=False):
    """((dst0 or 0) + slab 0) + slab 1 + ... in float32, on the device of the slabs.  ``reverse``: the mistake of the opposite order"""
    acc = torch.zeros_like(slabs[0], dtype=F32) if dst0 is None else dst0.to(F32).clone()
    for s in (reversed(range(len(slabs))) if reverse else range(len(slabs))):
        acc = acc + slabs[s].to(F32)
    return acc


def fold(slabs, mags, dst0=None):
    """the float64 sum of float64 slabs and of their magnitudes"""
    w, m = torch.stack(list(slabs)).sum(0), torch.stack(list(mags)).sum(0)
    return (w, m) if dst0 is None else (t64(dst0) + w, t64(dst0).abs() + m)


SLAB_COUNTS = [1, 7, 8, 9, 17]                        # 9 and 17: the second and third batch of eight loads
SLAB_GRID_CAP = 4096 * 256                            # float4 one lap of the capped grid covers (vf_sum_slabs_f32: 4096 blocks of 256 threads)
SLAB_N = [4, 1028, 4 * SLAB_GRID_CAP + 4]             # the last: one float4 past the capped grid (second lap), compared on the device


# ------------------------------------------------------------------ batched split-K of the forward kernel (ops.gemm_bf16_splitk)
def splitk(x, W, splits):
    """slab s = x[:, s ks : (s + 1) ks] @ W[s ks : (s + 1) ks] -> ([(value, magnitude)] per slab)"""
    ks = x.shape[1] // splits
    return [gemm(x[:, s * ks:(s + 1) * ks], W[s * ks:(s + 1) * ks]) for s in range(splits)]


def splitk_f32(x, W, splits, dst0=None):
    ks = x.shape[1] // splits
    return fold_f32([gemm_f32(x, W, k_range=(s * ks, (s + 1) * ks)) for s in range(splits)], dst0)


# ------------------------------------------------------------------ weight gradient (vf_gemm_tn_bf16)
TN_CHUNK = 64


def tn_chunks(M, splits, shift=0):
    """split s of S covers the 64-row chunks [floor(nc s / S), floor(nc (s + 1) / S)).  ``shift``: the mistake of a range moved by that
    many chunks (clipped to the matrix)"""
    nc = M // TN_CHUNK
    return [(min(nc, nc * s // splits + shift), min(nc, nc * (s + 1) // splits + shift)) for s in range(splits)]


def gemm_tn(x16, dy, splits, shift=0):
    """per split: dW = x16^T @ bf16_rne(dy) and db = the column sums of dy as it is stored (float32 unrounded, bf16 as it arrives), over
    the split's rows -> (dW [S][K][N], its magnitudes, db [S][N], its magnitudes)"""
    x, y16, y = x16.to(F64), as16(dy), t64(dy.float())
    dW, mW, db, mb = [], [], [], []
    for c0, c1 in tn_chunks(x.shape[0], splits, shift):
        r = slice(c0 * TN_CHUNK, c1 * TN_CHUNK)
        dW.append(x[r].t() @ y16[r])
        mW.append(x[r].abs().t() @ y16[r].abs())
        db.append(y[r].sum(0))
        mb.append(y[r].abs().sum(0))
    return torch.stack(dW), torch.stack(mW), torch.stack(db), torch.stack(mb)


def gemm_tn_f32(x16, dy, splits, unrounded_dy=False, db_rounded=False):
    """the kernel's order per split: 16 rows per matrix instruction inside 64-row chunks in order; db: row group g of 8 adds its rows
    g, g + 8, ... of every chunk in turn, the 8 groups are added in order.  The two flags are mistakes: products with the unrounded dy,
    and db summed from the rounded dy where dy arrives as float32 -> (dW [S][K][N], db [S][N]) float32"""
    x = x16.to(F32)
    y = dy.to(F32)
    y16 = y if unrounded_dy else as16(dy).to(F32)
    ys = y16 if db_rounded else y
    dW, db = [], []
    for c0, c1 in tn_chunks(x.shape[0], splits):
        acc = torch.zeros((x.shape[1], y.shape[1]), dtype=F32)
        grp = torch.zeros((8, y.shape[1]), dtype=F32)
        for c in range(c0, c1):
            for ms in range(0, TN_CHUNK, MFMA_K):
                r = slice(c * TN_CHUNK + ms, c * TN_CHUNK + ms + MFMA_K)
                acc = (acc.to(F64) + x[r].t().to(F64) @ y16[r].to(F64)).to(F32)
            blk = ys[c * TN_CHUNK:(c + 1) * TN_CHUNK].view(8, 8, -1)          # [j][group]: row group + 8 j
            for j in range(8):
                grp = grp + blk[j]
        s = torch.zeros(y.shape[1], dtype=F32)
        for g in range(8):
            s = s + grp[g]
        dW.append(acc)
        db.append(s)
    return torch.stack(dW), torch.stack(db)


# ------------------------------------------------------------------ the dispatcher and the tail policy, restated
def tail_policy(M, N, tail_on=True):
    """g256_tail_policy (csrc/gemm_bf16_g256.hip): (full row tiles, tail row tiles, 32-row blocks per wave group) per column of 256, or
    None for the plain grid.  Applied when the launch is more than one round of the 256 CUs, the last round holds 16 .. 184 tiles and the
    rows after whole rounds of full tiles fit one round of 128-row (ic 2) or 192-row (ic 3) tail tiles"""
    mt, nb = -(-M // 256), N // 256
    ntiles = mt * nb
    last = ntiles % 256
    if not tail_on or ntiles <= 256 or not 16 <= last <= 184:
        return None
    f = (ntiles // 256) * 256 // nb
    if f <= 0 or f >= mt:
        return None
    rem = -(-(M - f * 256) // 32)
    for ic in (2, 3):
        h = -(-rem // (2 * ic))
        if h * nb <= 256:
            return f, h, ic
    return None


def g256_takes(M, K, N, a16, o16, form, batch=1, lda=None, ldc=None, row0=0):
    """vf_gemm_bf16_g256_launch's conditions -> 'g256' or the code it returns"""
    f = FORMS[form]
    lda, ldc = K if lda is None else lda, N if ldc is None else ldc
    epi, res = f.get('epi'), bool(f.get('res')) or f.get('epi') == 'gelu_bwd'
    if not a16 or batch > 1 or N % 256 or K % 64 or M < 256 or lda & 7:
        return UNSUPPORTED
    if o16 and ((res and epi != 'gelu_bwd') or ldc & 1):
        return UNSUPPORTED
    if epi == 'gelu_bwd' and not o16:
        return UNSUPPORTED
    if epi == 'dual' and (res or ldc & 1):
        return UNSUPPORTED
    if f.get('gelu_grad') and not (f.get('res16') if epi == 'gelu_bwd' else (epi == 'dual' and o16)):
        return BAD_ARG
    if res and epi == 'gelu':
        return UNSUPPORTED
    if f.get('drop') and (o16 or epi is not None or row0 < 0 or row0 & 3 or ((M + row0 + 3) // 4) * N >= 2 ** 32):
        return UNSUPPORTED
    if M * lda * 2 >= 2 ** 31 or K * N * 2 >= 2 ** 31:
        return UNSUPPORTED
    return 'g256'


def forward_kernel(M, K, N, a16, o16, form, batch=1, lda=None, ldc=None, ldr=None, aux=None, g256_on=True, row0=0):
    """vf_gemm_bf16's decisions in its order -> 'staged', 'direct', 'g256', or the code of the refusal.  ``aux``: an out_aux pointer is
    passed (default: exactly when the form is a dual one)"""
    f = FORMS[form]
    epi, res = f.get('epi'), bool(f.get('res')) or f.get('epi') == 'gelu_bwd'
    lda, ldc, ldr = K if lda is None else lda, N if ldc is None else ldc, N if ldr is None else ldr
    aux = (epi == 'dual') if aux is None else aux
    if K % 64:
        return UNSUPPORTED
    if epi == 'gelu_bwd' and not o16:
        return UNSUPPORTED
    if (epi == 'dual') != aux:
        return BAD_ARG
    if lda < K or lda & 3 or ldc < N or (res and ldr < N):
        return BAD_ARG
    if epi == 'dual':
        if not a16 or batch > 1 or K % 128:
            return UNSUPPORTED
        return g256_takes(M, K, N, a16, o16, form, batch, lda, ldc, row0)
    if f.get('drop'):
        if not a16 or o16 or batch > 1 or K % 128:
            return UNSUPPORTED
        return g256_takes(M, K, N, a16, o16, form, batch, lda, ldc, row0)
    if a16 or o16:
        if K % 128 or batch > 1:
            return UNSUPPORTED
        if (a16 and lda & 7) or (o16 and res and epi != 'gelu_bwd'):
            return BAD_ARG
        if f.get('res16'):
            return g256_takes(M, K, N, a16, o16, form, batch, lda, ldc, row0)
        if g256_on:
            rc = g256_takes(M, K, N, a16, o16, form, batch, lda, ldc, row0)
            if rc != UNSUPPORTED:
                return rc
        return 'direct'
    return 'direct' if K % 128 == 0 and batch <= 1 else 'staged'


# ------------------------------------------------------------------ case tables
# the staged kernel: float32 x, K no multiple of 128.  M: one row, either side of the 128-row tile, three tiles with a ragged last one;
# N: half a column block, a ragged first block, one block, a ragged second block (8 and 72 columns)
STAGED_K = [64, 192]
STAGED_M = [1, 127, 128, 129, 300]
STAGED_N = [64, 72, 128, 136, 200]
STAGED_FORMS = ['none', 'bias', 'res', 'gelu_res']
STAGED_BATCHED = [(129, 72), (300, 200)]              # (M, N) of the batched form: K = 192 in 3 splits of one 64-deep chunk each
# leading dimensions: (lda - K for float32 x, lda - K for bf16 x, ldc - N, ldr - N); lda & 3 (& 7 for bf16 x) must be 0
PADS = [(0, 0, 0, 0), (4, 8, 3, 5)]

# the direct kernel, all four <A16, O16>: M below the 256-tile kernel's floor, and M = 300 where N is no multiple of 256.  N = 129: an odd
# width (the scalar bf16 store); N = 130 with ldc 131: the scalar store by the odd ldc; ldc 132: the paired store with a ragged block
DIRECT_K = [128, 384]
DIRECT_MN = [(M, N) for M in (1, 129, 255) for N in (64, 129, 130, 256)] + [(300, N) for N in (64, 129, 130)]
DIRECT_FORMS = {False: ['none', 'bias', 'res', 'gelu', 'gelu_res'], True: ['none', 'bias', 'gelu', 'gelu_bwd']}       # by o16


def direct_ldc(N):
    return [N, 131, 132] if N == 130 else [N, N + 3]


# the 256-tile kernel: one tile, one row / 255 rows / 128 rows in a second tile; two and six 64-deep stages; one and two column tiles
G256_M = [256, 257, 511, 640]
G256_K = [128, 384]
G256_N = [256, 512]
G256_FORMS = {False: ['bias', 'res', 'dual'],                                      # by o16
              True: ['bias', 'gelu', 'dual', 'dual_grad', 'gelu_bwd', 'gelu_bwd16', 'gelu_bwd16_grad']}
G256_DROPS = [(rate, row0, form) for rate in (0.5, 0.1) for row0 in (0, 8) for form in ('drop', 'drop_res')]
# (lda - K, ldc - N, ldr - N behind a float32 res / u, ldr - N behind a bf16 u or derivative table): the paired bf16 stores and loads of
# this kernel need an even ldc (the launcher refuses an odd one) and take an even ldr
G256_PADS = [(0, 0, 0, 0), (8, 6, 5, 6)]
G256_BOTH = (257, 384, 512)                         # the shape at which the 128-tile kernel runs against the same reference
DROP_SEED, DROP_SITE = 11, 2

# tail tiles: K = 128, N = 4096 (16 column tiles) -> the policy's tuple, by hand from g256_tail_policy: 4352 rows = 17 row tiles, 272
# tiles, 16 in the last round: one round of 16 full rows, 8 blocks left -> 2 tail rows of 128; 4282 rows: the same with 26 rows in the
# last tail tile; 6196 rows = 25 row tiles, 400 tiles, 144 in the last round: 16 full rows, 66 blocks left: 17 tail rows of 128 are 272
# tiles (more than a round), 11 of 192 are 176 -> ic 3, and the last tail tile holds 180 of its 192 rows
TAIL_K, TAIL_N = 128, 4096
TAIL_CASES = [(4352, (16, 2, 2)), (4282, (16, 2, 2)), (6196, (16, 11, 3))]
TAIL_FORMS = [('res', False), ('bias', True), ('dual', True), ('drop_res', False)]      # (form, o16)
TAIL_DROP = (0.1, 8)


def tail_rows(M, policy):
    """the rows compared against float64: the first 256, the 256 before the first tail tile, every tail row"""
    f0 = policy[0] * 256
    return torch.cat((torch.arange(0, 256), torch.arange(f0 - 256, M)))


# vf_gemm_tn_bf16 (M, K, N, splits): grids of 1, 1, 3, 5, 6 and 6 workgroups (the XCD remap's remainder branch: no multiple of 8), one
# chunk per split (320 rows in 5), uneven chunk ranges (5 chunks in 3: 1, 2, 2), two row tiles and three column tiles
TN_CASES = [(64, 256, 256, 1), (320, 256, 256, 1), (320, 256, 256, 3), (320, 256, 256, 5), (320, 512, 256, 3), (192, 256, 768, 2)]
TN_VARIANTS = [(y16, bias, record, pad) for y16 in (False, True) for bias in (False, True) for record in (False, True) for pad in (False, True)]
TN_PAD = 8

PACK_CASES = [(192, 200), (128, 256), (64, 72)]       # (K, N): K = 192 ends on a 64-deep chunk boundary that is no 128 boundary
