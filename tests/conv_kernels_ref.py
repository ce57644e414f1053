"""Test infrastructure of the per-kernel tests of the 3x3 convolution family (tests/test_hip_conv_kernels.py on the GPU,
tests/test_conv_kernels_ref_host.py on the CPU): the float64 reference, the two input classes, the case tables and a host mirror of the
dispatch conditions of the entry points.  Host only: nothing here touches the GPU or imports viewformer_amd.

Reference.  ``conv_ref`` states the three modes as vqgan_th.py defines them (stride 1 / pad 1; pad (0, 1, 0, 1) + stride 2 and no other
padding; nearest x2, then stride 1 / pad 1) on NCHW float64 and returns ``(value, magnitude)`` as NHWC rows [n Hout Wout][Cout], the
layout of the kernels' output.  The magnitude is the same expression with every summand replaced by its absolute value: the scale
rounding is judged against.  ``defect=...`` evaluates the same expression with one deliberate mistake (the discrimination controls of
the host file).

Inputs.  Exact class: activations are integers in [-4, 4], weights / bias / residual multiples of 2^-2 in [-1, 1], with planted exact
zeros and -0.0.  Every operand is exact in bf16 and in one fp16 piece, every product is a multiple of 2^-2 and every partial sum, in
any order, is a multiple of 2^-2 below 2^22 x 2^-2 (``EXACT_HEADROOM``; the host file asserts it on every row): exact in fp32.  Every
arm must return the reference as values.  Rounded class: the Gaussian draws of test_hip_x6.py / test_hip_bf16.py.

Case tables.  A row is ``(mode, Cin, Cout, Hin, Win, n)``; the tables are the point of these tests: non-square maps of one to four
8 x 16 tiles, chunk counts (Cin / 32) of 1, 2, 3, 5, 6, three 128-column blocks, absent bias / residual, strided output."""
import numpy as np
import torch
import torch.nn.functional as F

import training_kernels_ref as T

U = T.U
F64 = torch.float64
t64, rng, normal, mismatches, worst_ratio = T.t64, T.rng, T.normal, T.mismatches, T.worst_ratio

MODE_ID = {'s1': 1, 's2': 2, 'up': 3}                 # ops.MODE_CONV3_S1 / _S2PAD / _UP2
EXACT_HEADROOM = 2.0 ** 22                            # max(magnitude) / 2^-2 stays below this
X6_MAX, X6_RMS = 6e-7, 1.25                           # the x6 / x3h standing claim: max error < 6e-7 of magnitude, rms < 1.25 x native f32 + 1e-9
BF16_REL, BF16_REL_PRO = 3e-5, 3e-3                   # the bf16 arm's standing rule (max |error| / max |reference| on bf16-rounded operands)
GN_MEAN_TOL, GN_SCALE_TOL = 2e-6, 5e-6                # fused statistics: |mean error| < 2e-6 (1 + max |mean|), relative scale error < 5e-6
WGRAD_REL = 2e-6                                      # the weight gradient's standing whole-tensor bound


def out_hw(mode, H, W):
    return (H // 2, W // 2) if mode == 's2' else (2 * H, 2 * W) if mode == 'up' else (H, W)


def row_seed(row):
    mode, cin, cout, H, W, n = row[:6]
    return 7919 * MODE_ID[mode] + 31 * cin + 17 * cout + 13 * H + 11 * W + 5 * n


def to_rows(y):
    """NCHW -> NHWC rows [n H W][C]"""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def to_nchw(rows, n, H, W):
    return rows.view(n, H, W, -1).permute(0, 3, 1, 2)


# ------------------------------------------------------------------ the reference
DEFECTS = ('swap_hw', 'taps', 's2_pad', 'up_odd')


def _conv(a, w, mode, defect=None):
    """the convolution proper on NCHW.  Defects: 'taps' = ky <-> kx; 's2_pad' = the stride-2 pad on the left / top; 'up_odd' = the
    upsample reads source (y + 1) >> 1 (the odd copy of every source row / column is dropped, the next one taken)"""
    if defect == 'taps':
        w = w.transpose(2, 3)
    if mode == 'up':
        if defect == 'up_odd':
            H, W = a.shape[2], a.shape[3]
            iy = ((torch.arange(2 * H) + 1) // 2).clamp(max=H - 1)
            ix = ((torch.arange(2 * W) + 1) // 2).clamp(max=W - 1)
            a = a[:, :, iy][:, :, :, ix]
        else:
            a = F.interpolate(a, scale_factor=2.0, mode='nearest')
    if mode == 's2':
        return F.conv2d(F.pad(a, (1, 0, 1, 0) if defect == 's2_pad' else (0, 1, 0, 1)), w, None, stride=2)
    return F.conv2d(a, w, None, padding=1)


def _swap_hw(x):
    """the NHWC buffer of an n x H x W map read as n x W x H (the geometry's H and W exchanged)"""
    n, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(n, W, H, C).permute(0, 3, 1, 2)


def conv_ref(x_nchw64, w64, bias64, res64, mode, defect=None):
    """-> (value, magnitude), float64 rows [n Hout Wout][Cout]; ``bias64`` [Cout] / ``res64`` rows or None"""
    x, w = t64(x_nchw64), t64(w64)
    if defect == 'swap_hw':
        x = _swap_hw(x)
    ref, mag = to_rows(_conv(x, w, mode, defect)), to_rows(_conv(x.abs(), w.abs(), mode, defect))
    if bias64 is not None:
        ref, mag = ref + t64(bias64), mag + t64(bias64).abs()
    if res64 is not None:
        ref, mag = ref + t64(res64), mag + t64(res64).abs()
    return ref, mag


def conv_f32(x_nchw, w, bias, res, mode):
    """the float32 CPU restatement of the same expression (calibration basis of the native f32 arms)"""
    y = to_rows(_conv(x_nchw.float(), w.float(), mode))
    if bias is not None:
        y = y + bias.float()
    return y + res.float() if res is not None else y


def prologue(x_nchw, mean_c, scale_c, beta, swish, dtype=F64):
    """GroupNorm-apply (+ swish) with the float32 statistics the kernel is handed, evaluated in ``dtype``"""
    n, C = x_nchw.shape[:2]
    a = (x_nchw.to(dtype) - mean_c.to(dtype).view(n, C, 1, 1)) * scale_c.to(dtype).view(n, C, 1, 1) + beta.to(dtype).view(1, C, 1, 1)
    return a * torch.sigmoid(a) if swish else a


def gn_stats64(rows, gamma, n, HW, C, groups=32, eps=1e-6):
    """float64 (mean, rstd gamma) [n][C] of a stored [n HW][C] output"""
    mean, rstd = T.groupnorm_stats(rows, n, HW, C, groups, eps)
    cg = C // groups
    return mean.repeat_interleave(cg, 1), rstd.repeat_interleave(cg, 1) * t64(gamma)


def gn_stats_f32(x_rows, gamma, n, HW, C):
    """the float32 rounding of the float64 statistics, for the channel counts ops.groupnorm_stats refuses (96, 160, 192)"""
    mean_c, scale_c, _ = T.gn_stats_f32(x_rows, gamma, n, HW, C, 32)
    return mean_c, scale_c


def gn_stats_supported(C):
    """ops.groupnorm_stats takes C / 4 dividing 256 (test_hip_training_kernels.py, the header)"""
    return C % 4 == 0 and 256 % (C // 4) == 0


def conv_grads(x_nchw, w, dy_rows, mode, dtype=F64, defect=None, absolute=False):
    """autograd of sum(conv(x, w) dy): -> (dW as nine tap blocks [9][Cin][Cout] (tap = ky 3 + kx), db [Cout], dX rows [n Hin Win][Cin]);
    ``absolute``: every operand replaced by its absolute value = the magnitudes of the three.  dy and dX are flat NHWC buffers, so the
    H / W exchange ('swap_hw') needs the input reinterpreted only: the output's shape follows and both row views are taken from it"""
    fix = (lambda t: t.abs()) if absolute else (lambda t: t)
    if defect == 'swap_hw':                           # the x, dy and dX buffers all read as n x W x H
        x_nchw = _swap_hw(x_nchw)
    xv = fix(x_nchw.to(dtype)).clone().requires_grad_(True)
    wv = fix(w.to(dtype)).clone().requires_grad_(True)
    y = _conv(xv, wv, mode, defect)
    dy = fix(to_nchw(dy_rows.to(dtype), y.shape[0], y.shape[2], y.shape[3]))
    (y * dy).sum().backward()
    cout, cin = w.shape[:2]
    return wv.grad.permute(2, 3, 1, 0).reshape(9, cin, cout), dy.sum((0, 2, 3)), to_rows(xv.grad)


# ------------------------------------------------------------------ inputs
def _quarter(shape, g):
    return (g.integers(-4, 5, size=shape) / 4.0).astype(np.float32)


def _plant(a, g):
    f = a.reshape(-1)
    k = max(1, f.size // 16)
    f[g.integers(0, f.size, size=k)] = 0.0
    f[g.integers(0, f.size, size=max(1, k // 4))] = -0.0
    return a


def exact_inputs(row):
    """-> x [n][Cin][Hin][Win] integers in [-4, 4], w OIHW / bias / res rows: multiples of 2^-2 in [-1, 1]; zeros and -0.0 planted"""
    mode, cin, cout, H, W, n = row[:6]
    Ho, Wo = out_hw(mode, H, W)
    g = rng(row_seed(row))
    x = _plant(g.integers(-4, 5, size=(n, cin, H, W)).astype(np.float32), g)
    w = _plant(_quarter((cout, cin, 3, 3), g), g)
    b, r = _quarter((cout,), g), _plant(_quarter((n * Ho * Wo, cout), g), g)
    return tuple(torch.from_numpy(v) for v in (x, w, b, r))


def rounded_inputs(row):
    """the draws of test_hip_x6.py: -> x NCHW, w, bias, res rows, gamma, beta"""
    mode, cin, cout, H, W, n = row[:6]
    Ho, Wo = out_hw(mode, H, W)
    s = row_seed(row)
    return (normal((n, cin, H, W), s + 1, 1.5, 0.2), normal((cout, cin, 3, 3), s + 2, 0.05), normal((cout,), s + 3),
            normal((n * Ho * Wo, cout), s + 6), normal((cin,), s + 4, 0.3, 1.0), normal((cin,), s + 5, 0.2))


def grad_inputs(row):
    """-> x NCHW, w OIHW, dy rows [n Hout Wout][Cout]"""
    mode, cin, cout, H, W, n = row[:6]
    Ho, Wo = out_hw(mode, H, W)
    s = row_seed(row)
    return normal((n, cin, H, W), s + 11), normal((cout, cin, 3, 3), s + 12, 0.05), normal((n * Ho * Wo, cout), s + 13)


# ------------------------------------------------------------------ case tables: (mode, Cin, Cout, Hin, Win, n)
# halo geometries x channels (no full cross product): every geometry meets an odd chunk count above one (96 / 160) and an even one
# (64 / 192); every channel pair meets s1, up and s2; n is 1 on some rows and 2 or 3 on others.  Tiles: 1, 1x3, 3x1, 2x2.
HALO_ROWS = [
    ('s1', 32, 128, 8, 16, 1), ('s1', 96, 128, 8, 16, 2), ('s1', 64, 384, 8, 16, 1),
    ('s1', 160, 256, 8, 48, 1), ('s1', 192, 128, 8, 48, 1),
    ('s1', 96, 128, 24, 16, 1), ('s1', 64, 384, 24, 16, 2),
    ('s1', 160, 256, 16, 32, 1), ('s1', 192, 128, 16, 32, 2),                       # the largest row
    ('up', 32, 128, 4, 8, 2), ('up', 96, 128, 4, 8, 1), ('up', 192, 128, 4, 8, 1),
    ('up', 160, 256, 4, 24, 1), ('up', 64, 384, 4, 24, 1),
    ('up', 96, 128, 12, 8, 2), ('up', 192, 128, 12, 8, 1),
    ('s2', 32, 128, 16, 32, 1), ('s2', 160, 256, 16, 32, 2), ('s2', 192, 128, 16, 32, 1),
    ('s2', 96, 128, 16, 96, 1), ('s2', 64, 384, 16, 96, 1),
    ('s2', 160, 256, 48, 32, 1), ('s2', 64, 384, 48, 32, 2),
    ('s1', 96, 128, 8, 8, 3), ('s1', 64, 384, 8, 8, 3),                             # pair tiles, odd image count
    ('s2', 160, 256, 16, 16, 3), ('s2', 192, 128, 16, 16, 3),                       # stride-2 pair tiles (x3h only)
    ('s1', 32, 1024, 8, 16, 1),
]
# the per-tap kernel: shapes the halo path refuses
TAP_ROWS = [
    ('s1', 32, 3, 5, 7, 2), ('s1', 96, 130, 5, 7, 1),
    ('s2', 96, 5, 6, 10, 2), ('s2', 32, 160, 6, 10, 1),
    ('s2', 32, 130, 7, 5, 2), ('s2', 96, 3, 7, 5, 1),                               # odd input: the pad column / row is never read
    ('up', 96, 160, 3, 5, 1), ('up', 32, 5, 3, 5, 2),
]
# epilogue variants, every arm on the rows it accepts: bias / residual absent, strided output and residual (ldc = Cout + 4, ldr = Cout + 8)
# (x3h: 96 chunks odd -> 32x32x16 on both selector values; 192 -> the 16x16x32 kernel and its own epilogue; upsample; stride-2 tile)
EPI_ROWS = [('s1', 96, 128, 24, 16, 1), ('s1', 192, 128, 8, 48, 1), ('up', 64, 384, 4, 24, 1), ('s2', 160, 256, 16, 32, 1), ('s1', 96, 130, 5, 7, 1)]
EPI_VARIANTS = ('no_bias', 'no_res', 'neither', 'strided')
# rounded class: (row, prologue) with prologue in None / 'swish' / 'lin'; a stride-2 row with a prologue is refused by x6 / x3h
ROUNDED_ROWS = [(r, None if r[0] == 's2' else (None, 'swish', 'lin')[i % 3]) for i, r in enumerate(HALO_ROWS[:-1])] + [
    (('s2', 96, 128, 16, 96, 1), 'swish'), (('s1', 96, 130, 5, 7, 1), 'swish'), (('s2', 32, 130, 7, 5, 2), 'lin'), (('up', 96, 160, 3, 5, 1), None)]
# fused statistics: Cout / 32 = 4, 8, 32 on non-square maps.  32 -> 1024 leaves the 16x16x32 x3h kernel through its odd chunk count
# already, so the Cout / 32 > 16 fork proper is met by 64 -> 1024
STATS_ROWS = [('s1', 64, 128, 8, 48, 2), ('up', 96, 256, 4, 24, 1), ('s2', 64, 128, 16, 96, 2), ('s1', 32, 1024, 8, 16, 1),
              ('s1', 64, 1024, 8, 16, 1), ('s1', 64, 256, 8, 8, 3)]
STATS_REFUSED = ('s1', 64, 384, 8, 16, 1)             # Cout / 32 = 12: no fused statistics
# weight gradient: P = n Hout Wout = 1024 -> two slabs
WGRAD_ROWS = [('s2', 128, 128, 32, 64, 2), ('up', 128, 128, 8, 16, 2), ('s1', 256, 132, 16, 64, 1)]
# dX through VQGANTrainer._conv_dx: (mode, cin, cout, Hin, Win, n) of the FORWARD convolution
DX_ROWS = [(m, ci, co, H, W, n) for m in ('s1', 's2', 'up') for (ci, co, H, W, n) in ((128, 32, 8, 16, 2), (32, 128, 16, 8, 1), (32, 128, 8, 16, 1),
                                                                                     (128, 32, 16, 8, 2))] + [
    ('s1', 128, 3, 8, 16, 2), ('s1', 32, 3, 16, 8, 1), ('up', 128, 3, 4, 8, 1), ('s2', 128, 32, 6, 10, 2), ('s2', 32, 3, 6, 10, 1)]

FORWARD_ROWS = list(dict.fromkeys(HALO_ROWS + TAP_ROWS + EPI_ROWS + [r for r, _ in ROUNDED_ROWS] + STATS_ROWS + [STATS_REFUSED]))


# ------------------------------------------------------------------ host mirror of the dispatch conditions
CK, BN, TH, TW = 32, 128, 8, 16                       # conv3_halo_*.hip: channel chunk, column block, tile
ARMS = ('f32', 'x6', 'x3h', 'x3h_k16', 'bf16', 'bf16_16')


def _halo(Ho, Wo):
    return Ho % TH == 0 and Wo % TW == 0


def _gn_ok(cout):
    return cout % 32 == 0 and cout // 32 in (4, 8, 16, 32)                          # halo_common.h:27-28 (vf_halo_gn_check)


def arm_accepts(arm, row, pro=False, gn=False):
    """does the entry point behind ``arm`` take the row (else it returns VF_ERR_UNSUPPORTED -> VfError)"""
    mode, cin, cout, H, W, n = row[:6]
    Ho, Wo = out_hw(mode, H, W)
    if arm == 'f32':                                                                # igemm_f32.hip:352-354: any shape with Cin % 32 == 0, never statistics
        return cin % CK == 0 and not gn
    if cin % CK or cout % BN or (gn and not _gn_ok(cout)):
        return False
    pair = mode == 's1' and (Ho, Wo) == (8, 8)
    if mode == 's2':
        if arm in ('bf16', 'bf16_16'):                                              # conv3_halo_bf16.hip:547
            return False
        p8 = arm in ('x3h', 'x3h_k16') and (Ho, Wo) == (8, 8)                       # conv3_halo_x3h.hip:851-852, conv3_halo_x6.hip:432
        return (p8 or _halo(Ho, Wo)) and not pro
    if arm == 'bf16_16' and pair:                                                   # conv3_halo_bf16.hip:559
        return False
    return pair or _halo(Ho, Wo)                                                    # conv3_halo_x6.hip:442-443, _x3h.hip:867-868, _bf16.hip:548-549


def f32_kernel(row):
    """which kernel vf_igemm_f32 runs: conv3_halo_f32.hip:271-277 (vf_conv3_halo_try), else the per-tap kernel"""
    mode, cin, cout, H, W, n = row[:6]
    Ho, Wo = out_hw(mode, H, W)
    pair = mode == 's1' and (Ho, Wo) == (8, 8)
    return 'halo_f32' if mode in ('s1', 'up') and cout % BN == 0 and cin % CK == 0 and (pair or _halo(Ho, Wo)) else 'tap'


def x3h_kernel(row, pro=False, gn=False, k32=1):
    """which kernel vf_conv3_halo_x3h launches for an accepted row: conv3_halo_x3h.hip:857-864 (stride 2), :877-878 and dispatch_pro :812-818"""
    mode, cin, cout, H, W, n = row[:6]
    Ho, Wo = out_hw(mode, H, W)
    if mode == 's2':
        return 's2_pair' if (Ho, Wo) == (8, 8) else 's2_tile'
    pair = mode == 's1' and (Ho, Wo) == (8, 8)
    lds = 2 * (10 * 18 + 1) * 144 + 6 * 4096 - 1024 + 3 * (cin if pro else 0) * 4   # :790 with Geo<false, false> (:48-53)
    if mode != 'up' and not pair and (cin // CK) % 2 == 0 and (not gn or cout // 32 <= 16) and lds <= 80 * 1024 and k32:
        return 'k32'                                                                # the 16x16x32 kernel
    return 'k16_pair' if pair else 'k16_up' if mode == 'up' else 'k16'


def wgrad_splits(row):
    """train_ops.conv3_wgrad: tiles and slabs"""
    mode, cin, cout, H, W, n = row[:6]
    Ho, Wo = out_hw(mode, H, W)
    P = n * Ho * Wo
    tiles = (9 * (cin // 128) + 1) * ((cout + 127) // 128)
    return max(1, min(256, 512 // tiles, P // 512))
