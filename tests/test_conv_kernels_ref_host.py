"""CPU: the float64 convolution reference of tests/conv_kernels_ref.py pinned against an independent statement (nine shifted slices
multiplied and added in numpy float64, no conv2d) on every row of the tables; the exact class's fp32 headroom; the discrimination
controls (a reference with H and W exchanged, the taps transposed, the stride-2 pad on the left / top, or the upsample's odd copy
dropped must land at least 1000 tolerances away on every row); the coverage of the kernels' dispatch forks by the tables; and the
calibration the constants of tests/test_hip_conv_kernels.py come from: the float32 CPU restatement of the native f32 arms, the
weight-gradient tap blocks and dX against float64 on the GPU test's own inputs, in units of 2^-24 x magnitude."""
import numpy as np
import pytest
import torch

import conv_kernels_ref as R


def _id(row):
    return '-'.join(str(v) for v in row)


# ------------------------------------------------------------------ 1. the reference is pinned
def _nine_slices(x, w, mode):
    """x [n][C][H][W], w [Co][C][3][3] numpy float64 -> [n Ho Wo][Co]: out = sum over (ky, kx) of slice(ky, kx) . w[:, :, ky, kx]"""
    if mode == 'up':
        x = x.repeat(2, axis=2).repeat(2, axis=3)
    n, C, H, W = x.shape
    if mode == 's2':
        xp, s, Ho, Wo = np.pad(x, ((0, 0), (0, 0), (0, 1), (0, 1))), 2, H // 2, W // 2
    else:
        xp, s, Ho, Wo = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1))), 1, H, W
    out = np.zeros((n * Ho * Wo, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]
            assert sl.shape == (n, C, Ho, Wo)
            out += sl.transpose(0, 2, 3, 1).reshape(-1, C) @ w[:, :, ky, kx].T
    return out


@pytest.mark.parametrize('row', R.FORWARD_ROWS, ids=_id)
def test_conv_ref_against_nine_shifted_slices(row):
    x, w, b, res, _, _ = R.rounded_inputs(row)
    ref, mag = R.conv_ref(x, w, b, res, row[0])
    xn, wn = x.double().numpy(), w.double().numpy()
    want = _nine_slices(xn, wn, row[0]) + b.double().numpy() + res.double().numpy()
    wmag = _nine_slices(np.abs(xn), np.abs(wn), row[0]) + np.abs(b.double().numpy()) + np.abs(res.double().numpy())
    Ho, Wo = R.out_hw(row[0], row[3], row[4])
    assert ref.shape == (row[5] * Ho * Wo, row[2])
    assert float((ref - torch.from_numpy(want)).abs().max()) <= 1e-12 * float(mag.max())
    assert float((mag - torch.from_numpy(wmag)).abs().max()) <= 1e-12 * float(mag.max())
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('row', list(dict.fromkeys(R.HALO_ROWS + R.TAP_ROWS + R.EPI_ROWS)), ids=_id)
def test_exact_class_has_fp32_headroom(row):
    """operands on their grids, zeros and -0.0 present, the reference a multiple of 2^-2, max(magnitude) / 2^-2 < 2^22: every partial
    sum in any order is exact in fp32; the operands are exact in bf16 (and so in one fp16 piece: at most 3 significant bits)"""
    x, w, b, res = R.exact_inputs(row)
    for t, step in ((x, 1.0), (w, 0.25), (b, 0.25), (res, 0.25)):
        assert bool((t / step == (t / step).round()).all()) and float(t.abs().max()) <= (4.0 if step == 1.0 else 1.0)
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t)
    assert int((x == 0).sum()) > 0 and bool(torch.signbit(x[x == 0]).any()) and int((w == 0).sum()) > 0
    ref, mag = R.conv_ref(x, w, b, res, row[0])
    assert float(mag.max()) / 0.25 < R.EXACT_HEADROOM
    assert bool((ref * 4 == (ref * 4).round()).all())
    assert bool((ref.float().double() == ref).all())


# ------------------------------------------------------------------ 2. discrimination controls
def _defects(row):
    mode, H, W = row[0], row[3], row[4]
    return [d for d in R.DEFECTS if (d != 'swap_hw' or H != W) and (d != 's2_pad' or mode == 's2') and (d != 'up_odd' or mode == 'up')]


def _tol_f32():
    import test_hip_conv_kernels as G
    return max(R.X6_MAX, max(G.C.values()) * R.U)


@pytest.mark.parametrize('row', R.FORWARD_ROWS, ids=_id)
def test_a_defective_reference_is_told_apart(row):
    """rounded class: every defect is at least 1000 x the per-element tolerance (the larger of 6e-7 and c 2^-24, of the magnitude) away
    on some element, and at least 1000 x 3e-5 of max |reference| (the bf16 rule without the prologue).  The bf16 rule WITH the prologue,
    3e-3 of max |reference|, cannot be exceeded a thousandfold by any output at all (that would be three times the largest value): there
    the control asks for 100 x, 0.3 of the largest value.  Exact class: at least one element differs.  Non-square rows run all defects
    that apply to their mode; square rows (the 8x8 pair tiles) all but the H / W exchange"""
    mode = row[0]
    assert row[3] != row[4] or (row[3], row[4]) in ((8, 8), (16, 16))
    x, w, b, res, _, _ = R.rounded_inputs(row)
    ref, mag = R.conv_ref(x, w, b, res, mode)
    xe, we, be, re_ = R.exact_inputs(row)
    refe, _ = R.conv_ref(xe, we, be, re_, mode)
    tol = _tol_f32()
    ds = _defects(row)
    assert 'taps' in ds and (row[3] == row[4] or 'swap_hw' in ds)
    for d in ds:
        bad, _ = R.conv_ref(x, w, b, res, mode, defect=d)
        worst = float(((bad - ref).abs() / mag).max())
        rel = float((bad - ref).abs().max() / ref.abs().max())
        assert worst >= 1000 * tol, (row, d, worst)
        assert rel >= 1000 * R.BF16_REL and rel >= 100 * R.BF16_REL_PRO, (row, d, rel)
        assert R.mismatches(R.conv_ref(xe, we, be, re_, mode, defect=d)[0], refe) > 0, (row, d)


@pytest.mark.parametrize('row', R.WGRAD_ROWS + R.DX_ROWS, ids=_id)
def test_a_defective_gradient_is_told_apart(row):
    """the same controls on the gradients (the x, dy and dX buffers read as n x W x H for the exchange): every tap block of dW moves but
    those a defect leaves in place by construction (the diagonal ones under a tap transposition, the centre one of a stride-1 row under the
    exchange); dX moves"""
    import test_hip_conv_kernels as G
    x, w, dy = R.grad_inputs(row)
    dW, db, dX = R.conv_grads(x, w, dy, row[0])
    mW, mb, mX = R.conv_grads(x, w, dy, row[0], absolute=True)
    assert row[3] != row[4]
    for d in _defects(row):
        bW, _, bX = R.conv_grads(x, w, dy, row[0], defect=d)
        if row in R.WGRAD_ROWS:
            moved = [t for t in range(9) if float(((bW[t] - dW[t]).abs() / mW[t]).max()) >= 1000 * G.C['wgrad'] * R.U]
            # (the centre tap at stride 1 pairs x and dy at the same flat position whatever the geometry: the exchange leaves that block in place)
            must = {1, 2, 3, 5, 6, 7} if d == 'taps' else set(range(9)) - {4} if (d, row[0]) == ('swap_hw', 's1') else set(range(9))
            assert set(moved) >= must, (row, d, moved)
        else:
            assert float(((bX - dX).abs() / mX).max()) >= 1000 * G.C['dx'] * R.U, (row, d)


# ------------------------------------------------------------------ 3. the tables reach every fork of the dispatch
def test_tables_cover_the_dispatch_forks():
    rows = R.HALO_ROWS
    ok = lambda arm, **kw: [r for r in rows if R.arm_accepts(arm, r, **kw)]           # noqa: E731
    pair = lambda r: r[0] == 's1' and (r[3], r[4]) == (8, 8)                          # noqa: E731
    for arm in ('x6', 'x3h', 'bf16'):                                                 # pair / not pair, UP2 (conv3_halo_x6.hip:452-453, _x3h.hip:877-878, _bf16.hip:560-561)
        acc = ok(arm)
        assert any(pair(r) for r in acc) and any(r[0] == 's1' and not pair(r) for r in acc) and any(r[0] == 'up' for r in acc)
    assert {R.f32_kernel(r) for r in rows + R.TAP_ROWS} == {'halo_f32', 'tap'}
    kinds = {R.x3h_kernel(r) for r in ok('x3h')}
    assert kinds == {'s2_pair', 's2_tile', 'k32', 'k16', 'k16_up', 'k16_pair'}        # conv3_halo_x3h.hip:857-864 and :812-818
    assert any(R.arm_accepts('x6', r) for r in rows if r[0] == 's2')                  # conv3_halo_x6.hip:431-439
    assert not any(R.arm_accepts('x6', r) for r in rows if r[0] == 's2' and (r[3], r[4]) == (16, 16))
    for geo in {(r[0], r[3], r[4]) for r in rows[:-1]}:                               # every geometry: an odd chunk count above one and an even one
        chunks = {r[1] // R.CK for r in rows if (r[0], r[3], r[4]) == geo}
        assert any(c % 2 == 1 and c > 1 for c in chunks) and any(c % 2 == 0 for c in chunks), geo
    for pairc in {(r[1], r[2]) for r in rows[:-1]}:                                   # every channel pair: s1, up, s2
        assert {r[0] for r in rows if (r[1], r[2]) == pairc} == {'s1', 'up', 's2'}, pairc
    assert {(r[1], r[2]) for r in rows[:-1]} == {(32, 128), (96, 128), (160, 256), (64, 384), (192, 128)}
    assert {r[5] for r in rows} >= {1, 2, 3}
    assert any(r[2] // R.BN == 3 for r in rows)                                       # three column blocks
    # odd chunk count above one / even chunk count on the 16x16x32 fork (conv3_halo_x3h.hip:812)
    s1 = [r for r in ok('x3h') if r[0] == 's1' and not pair(r)]
    assert any(R.x3h_kernel(r) == 'k16' and (r[1] // R.CK) % 2 == 1 and r[1] // R.CK > 1 for r in s1)
    assert any(R.x3h_kernel(r) == 'k32' for r in s1) and all(R.x3h_kernel(r, k32=0) != 'k32' for r in s1)
    # Cout / 32 > 16 with statistics: an EVEN chunk count that leaves the 16x16x32 kernel for this reason alone
    st = [r for r in R.STATS_ROWS if R.arm_accepts('x3h', r, gn=True)]
    assert any(r[2] // 32 > 16 and R.x3h_kernel(r, gn=False) == 'k32' and R.x3h_kernel(r, gn=True) == 'k16' for r in st)
    assert any(R.x3h_kernel(r, gn=True) == 'k32' for r in st) and any(R.x3h_kernel(r, gn=True) == 's2_tile' for r in st)
    assert {r[2] for r in R.STATS_ROWS} >= {128, 256, 1024} and all(r[3] != r[4] for r in R.STATS_ROWS[:5])
    assert not any(R.arm_accepts(a, R.STATS_REFUSED, gn=True) for a in R.ARMS) and R.arm_accepts('x6', R.STATS_REFUSED)
    # the per-tap table: shapes every halo arm refuses
    assert all(not R.arm_accepts(a, r) for r in R.TAP_ROWS for a in R.ARMS[1:]) and all(R.arm_accepts('f32', r) for r in R.TAP_ROWS)
    assert {r[1] for r in R.TAP_ROWS} == {32, 96} and {r[2] for r in R.TAP_ROWS} == {3, 5, 130, 160}
    # every arm meets an epilogue row, all of them non-square
    for arm in R.ARMS:
        assert any(R.arm_accepts(arm, r) for r in R.EPI_ROWS)
    for k32, kinds in ((1, {'k32', 'k16', 'k16_up', 's2_tile'}), (0, {'k16', 'k16_up', 's2_tile'})):     # by kernel, not by arm name
        assert {R.x3h_kernel(r, k32=k32) for r in R.EPI_ROWS if R.arm_accepts('x3h', r)} == kinds
    assert {R.f32_kernel(r) for r in R.EPI_ROWS} == {'halo_f32', 'tap'} and any(R.arm_accepts('x6', r) and r[0] == 's2' for r in R.EPI_ROWS)
    assert all(r[3] != r[4] for r in R.EPI_ROWS)
    # the weight gradient's slab sum: the product's own rule (train_ops.conv3_wgrad_splits), which the table's mirror must follow
    from viewformer_amd import train_ops
    for r in R.WGRAD_ROWS:
        Ho, Wo = R.out_hw(r[0], r[3], r[4])
        assert train_ops.conv3_wgrad_splits(r[1], r[2], r[5] * Ho * Wo) == R.wgrad_splits(r) == 2
    assert all(((9 * r[1] + 1) * r[2]) % 4 == 0 for r in R.WGRAD_ROWS)
    assert any(r[2] % 32 for r in R.DX_ROWS) and {r[0] for r in R.DX_ROWS} == {'s1', 's2', 'up'}


# ------------------------------------------------------------------ 4. calibration
def calibration():
    """quantity -> worst |float32 restatement - float64| / (2^-24 x magnitude) over the GPU test's inputs"""
    out = {}

    def note(k, got, want, mag):
        out[k] = max(out.get(k, 0.0), R.worst_ratio(got, want, mag))
    for row, pro in R.ROUNDED_ROWS:
        mode, cin, cout, H, W, n = row
        x, w, b, res, gamma, beta = R.rounded_inputs(row)
        a64, a32 = x.double(), x
        if pro:
            mean_c, scale_c = R.gn_stats_f32(R.to_rows(x), gamma, n, H * W, cin)
            a64 = R.prologue(x, mean_c, scale_c, beta, pro == 'swish')
            a32 = R.prologue(x, mean_c, scale_c, beta, pro == 'swish', dtype=torch.float32)
        ref, mag = R.conv_ref(a64, w, b, res, mode)
        note(R.f32_kernel(row), R.conv_f32(a32, w, b, res, mode), ref, mag)
    for row in R.WGRAD_ROWS + R.DX_ROWS:
        x, w, dy = R.grad_inputs(row)
        dW, db, dX = R.conv_grads(x, w, dy, row[0])
        mW, mb, mX = R.conv_grads(x, w, dy, row[0], absolute=True)
        gW, gb, gX = R.conv_grads(x, w, dy, row[0], dtype=torch.float32)
        if row in R.WGRAD_ROWS:
            note('wgrad', gW, dW, mW)
            note('wgrad', gb, db, mb)
        else:
            note('dx', gX, dX, mX)
    return out


def _pow2_ceil(v):
    return 2.0 ** int(np.ceil(np.log2(max(v, 2.0 ** -20))))


def test_calibration_covers_the_gpu_tests_constants():
    """c = 4 x the float32 CPU restatement's worst error, rounded up to a power of two.  The restatement's own sums depend on how torch
    splits them, so the table may sit one binade from this run's figure, never further"""
    import test_hip_conv_kernels as G
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
        assert _pow2_ceil(4 * v) <= 2 * G.C[k] and G.C[k] <= 2 * _pow2_ceil(4 * v), (k, v, G.C[k])
