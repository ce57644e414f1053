"""CPU: the float64 references of tests/codec_kernels_ref.py pinned against independent statements (GroupNorm against
torch.nn.functional.group_norm in float64, attention against an explicit loop, the lookup against cdist, the small convolutions against
nine shifted slices, the byte pre-processing against the TF formula on all 256 values); the calibration the constants of
tests/test_hip_codec_kernels.py come from (the float32 CPU restatement of each kernel's summation order against float64 on the GPU
test's own inputs, in units of 2^-24 x magnitude, printed); the discrimination controls (every tolerance accepts the restatement and
rejects a planted defect on those inputs); and the caps the GPU test leans on (exempt share of the random lookup, the selector's
off-target mass, the planted margin, the exact classes' headroom, the sizes that reach a second lap / a fork / an LDS limit)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import codec_kernels_ref as K
import conv_kernels_ref as CR


def _id(row):
    return '-'.join(str(v) for v in row)


def _G():
    import test_hip_codec_kernels as G
    return G


# ------------------------------------------------------------------ 1. the references are pinned
@pytest.mark.parametrize('cls', ('n15', 'groups'))
@pytest.mark.parametrize('row', K.STATS_ROWS, ids=_id)
def test_groupnorm_ref_against_functional_group_norm(row, cls):
    Cc, groups, HW = row
    n = K.STATS_N
    x, gamma = K.stats_inputs(row, cls)
    beta = K.normal((Cc,), 5, 0.2)
    mean, var, rstd = K.gn_ref(x, n, HW, Cc, groups)
    mc, sc = K.gn_channels(mean, rstd, gamma, Cc)
    mine, mag = K.apply_ref(x.double(), mc, sc, beta, n, HW, Cc, False)
    want = F.group_norm(x.double().view(n, HW, Cc).permute(0, 2, 1), groups, gamma.double(), beta.double(), eps=K.EPS).permute(0, 2, 1).reshape(n * HW, Cc)
    assert float(((mine - want).abs() / mag.clamp_min(1e-30)).max()) < 1e-9
    # the partials of the restatement, combined in float64, are the same statistics to fp32 accuracy
    part = K.gn_partials_f32(x, n, HW, Cc, groups)
    m2, _, _ = K.finalize_ref(part, HW, Cc // groups)
    assert float((m2 - mean).abs().max()) <= 1e-4 * (1 + float(mean.abs().max()))


def test_swish_and_apply_ref_against_silu():
    row = K.APPLY_ROWS[4]
    Cc, HW, n = row
    x, mc, sc, beta = K.apply_inputs(row)
    got, _ = K.apply_ref(x, mc, sc, beta, n, HW, Cc, True)
    t = (x.double().view(n, HW, Cc) - mc.double().view(n, 1, Cc)) * sc.double().view(n, 1, Cc) + beta.double()
    assert float((got.view(n, HW, Cc) - F.silu(t)).abs().max()) < 1e-14
    tt = torch.linspace(-30, 30, 20001, dtype=torch.float64)
    g = torch.autograd.functional.jacobian(lambda u: K.swish(u).sum(), tt)
    assert float(g.abs().max()) <= K.SWISH_LIP


@pytest.mark.parametrize('cls', K.ATTN_CLASSES)
def test_attention_ref_against_an_explicit_loop(cls):
    HW, Cc, n = 64, 256, 1
    q, k, v = K.attn_inputs(cls, HW, Cc, n)
    scale = K.attn_scale(Cc)
    ref, M, S, p, _ = K.attn_ref(q, k, v, scale)
    qn, kn, vn = (t[0].double().numpy() for t in (q, k, v))
    for i in range(HW):
        s = np.array([float(np.dot(qn[i], kn[j])) * scale for j in range(HW)])
        e = np.exp(s - s.max())
        pi = e / e.sum()
        o = sum(pi[j] * vn[j] for j in range(HW))
        assert np.abs(o - ref[0, i].numpy()).max() <= 1e-12 * (1 + np.abs(vn).max())
        assert np.abs(sum(pi[j] * np.abs(vn[j]) for j in range(HW)) - M[0, i].numpy()).max() <= 1e-12 * (1 + np.abs(vn).max())
    # a strided layout read back with its own ld returns the operands
    ld = 3 * Cc + 8
    q2, k2, v2 = K.attn_unpack(K.attn_pack(q, k, v, ld), n, HW, Cc, ld)
    assert torch.equal(q2, q) and torch.equal(k2, k) and torch.equal(v2, v)


@pytest.mark.parametrize('row', K.LOOKUP_ROWS, ids=_id)
def test_lookup_ref_against_cdist(row):
    z, E = K.random_lookup_inputs(row)
    d = K.dist64(z, E)
    want = torch.cdist(z.double(), E.double().t()) ** 2
    assert float((d - want).abs().max()) <= 1e-12 * float(want.max())
    assert torch.equal(K.argmin_ref(z, E), want.argmin(1)) or float((want.gather(1, K.argmin_ref(z, E).view(-1, 1)).view(-1) - want.min(1).values).max()) < 1e-12


def _nine_slices(x, w):
    """x [n][H][W][C] zero-padded NHWC float64, w [Co][C][3][3] -> [n][H][W][Co]"""
    n, H, W, Cc = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((n, H, W, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].T
    return out


@pytest.mark.parametrize('row', K.CONV_IN_ROWS + [(c, n, H, W) for (n, H, W, c) in K.CONV_IN_X3H_ROWS], ids=_id)
def test_conv_in_ref_against_nine_shifted_slices(row):
    img, w, b = K.conv_in_inputs(row)
    ref, mag = K.conv_in_ref(img, w, b)
    x = K.preprocess_u8(img).double().numpy()
    want = _nine_slices(x, w.double().numpy()) + b.double().numpy()
    assert np.abs(ref.numpy() - want).max() <= 1e-12 * float(mag.max())
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('row', K.SMALL_ROWS, ids=_id)
def test_small_cout_ref_against_nine_shifted_slices(row):
    x, w, b, mc, sc, beta = K.small_inputs(row, False)
    n, cin, H, W = x.shape
    for pro in K.SMALL_PRO:
        p = None if pro is None else (mc, sc, beta)
        ref, mag, MAG = K.small_ref(x, w, b, p, pro == 'swish')
        a = x.double() if p is None else CR.prologue(x, mc, sc, beta, pro == 'swish')
        want = _nine_slices(a.permute(0, 2, 3, 1).numpy(), w.double().numpy()) + b.double().numpy()
        assert np.abs(ref.numpy() - want.reshape(n * H * W, -1)).max() <= 1e-12 * float(mag.max())
        assert bool((MAG >= mag).all()) and bool((mag >= ref.abs() * (1 - 1e-12)).all())


def test_byte_preprocessing_equals_the_tf_formula_on_all_256_values():
    from oracle import vqgan_oracle as vq
    b = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    mine = K.preprocess_u8(b)
    tf = (np.arange(256, dtype=np.uint8).astype(np.float32) * np.float32(1.0 / 255)) * np.float32(2) - np.float32(1)      # convert_image_dtype, * 2 - 1
    assert np.array_equal(mine[0, :, :, 0].reshape(-1).numpy(), tf)
    assert torch.equal(vq.preprocess_u8(b).permute(0, 2, 3, 1), mine)
    assert float(mine.min()) == -1.0 and float(mine.max()) == 1.0


# ------------------------------------------------------------------ 2. calibration
def calibration():
    """quantity -> worst |float32 restatement - float64| / (2^-24 x magnitude) over the GPU test's inputs"""
    out = {}

    def note(k, r):
        out[k] = max(out.get(k, 0.0), float(r))
    n = K.STATS_N
    for row in K.STATS_ROWS:
        Cc, groups, HW = row
        for cls in K.STATS_CLASSES:
            x, gamma = K.stats_inputs(row, cls)
            mean, var, _ = K.gn_ref(x, n, HW, Cc, groups)
            m2, v2, _ = K.finalize_ref(K.gn_partials_f32(x, n, HW, Cc, groups), HW, Cc // groups)
            note('gn_mean', K.worst_ratio(m2.float(), mean, mean.abs() + var.sqrt()))
            note('gn_var', K.worst_ratio(v2, var, mean * mean + var))
    for row in K.APPLY_ROWS:
        Cc, HW, n_ = row
        x, mc, sc, beta = K.apply_inputs(row)
        ref, mag = K.apply_ref(x, mc, sc, beta, n_, HW, Cc, False)
        note('apply', K.worst_ratio(K.apply_ref(x, mc, sc, beta, n_, HW, Cc, False, dtype=torch.float32)[0], ref, mag))
    for row in K.PRO_ROWS:
        inp = K.pro_inputs(row)
        for sw in (False, True):
            ref, mag, MAG = K.pro_ref(row, inp, sw)
            note('gemm_pro', K.worst_ratio(K.pro_f32(row, inp, sw), ref, MAG))
    for HW, Cc in K.ATTN_SHAPES:
        for cls in K.ATTN_CLASSES[1:]:
            q, k, v = K.attn_inputs(cls, HW, Cc, 3)
            scale = K.attn_scale(Cc)
            o32, s32 = K.attn_f32(q, k, v, scale)
            _, _, _, _, s64 = K.attn_ref(q, k, v, scale)
            smag = K.t64(q).abs() @ K.t64(k).abs().transpose(1, 2) * scale
            note(K.attn_score_key(cls), K.worst_ratio(s32, s64, smag))
            p = torch.softmax(s32.double(), -1)                  # the softmax and P V alone: float64 on the restatement's own scores
            note('attn_pv', K.worst_ratio(o32, p @ v.double(), p @ v.double().abs()))
    for D, Kc in K.CB_SHAPES:
        E = K.codebook(D, Kc)
        ref = E.double().pow(2).sum(0)
        note('colsumsq', K.worst_ratio(K.colsumsq_f32(E), ref, ref))
    for row in K.CONV_IN_ROWS:
        img, w, b = K.conv_in_inputs(row)
        for bias in (b, None):
            ref, mag = K.conv_in_ref(img, w, bias)
            note('conv_in', K.worst_ratio(K.conv_in_f32(img, w, bias), ref, mag))
    for row in K.SMALL_ROWS:
        for bf16 in (False, True):
            x, w, b, mc, sc, beta = K.small_inputs(row, bf16)
            for pro in K.SMALL_PRO:
                p = None if pro is None else (mc, sc, beta)
                ref, mag, MAG = K.small_ref(x, w, b, p, pro == 'swish')
                note('small', K.worst_ratio(K.small_f32(x, w, b, p, pro == 'swish'), ref, MAG))
    return out


@pytest.fixture(scope='module')
def cal():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return calibration()
    finally:
        torch.set_num_threads(threads)


def test_calibration_covers_the_gpu_tests_constants(cal):
    """c = 4 x the float32 CPU restatement's worst error, rounded up to a power of two.  The restatement's own sums depend on how torch
    splits them, so the table may sit one binade from this run's figure, never further"""
    G = _G()
    for k in sorted(cal):
        print(f'calibration {k}: fp32 CPU restatement worst {cal[k]:.2f} units of 2^-24 x magnitude -> c = {K.pow2_ceil(4 * cal[k]):g} (table: {G.C[k]:g})')
    assert set(cal) == set(G.C)
    for k, v in cal.items():
        assert K.pow2_ceil(4 * v) <= 2 * G.C[k] and G.C[k] <= 2 * K.pow2_ceil(4 * v), (k, v, G.C[k])


# ------------------------------------------------------------------ 3. every tolerance accepts the restatement and rejects a planted defect
@pytest.mark.parametrize('row', K.STATS_ROWS, ids=_id)
def test_statistics_tolerance_tells_the_defects(row):
    """the restatement passes on every class; a dropped last pixel of a split and the unbiased variance are rejected on the centred
    class (mean / std = 0), a missing eps on the per-group class (its smallest variances are 1e-3)"""
    G = _G()
    Cc, groups, HW = row
    n = K.STATS_N
    for cls in K.STATS_CLASSES:
        x, gamma = K.stats_inputs(row, cls)
        m2, v2, r2 = K.finalize_ref(K.gn_partials_f32(x, n, HW, Cc, groups), HW, Cc // groups)
        mc, sc = K.gn_channels(m2.float().double(), r2.float().double(), gamma, Cc)
        ok, wm, ws = K.stats_within(mc.float(), (sc.float()), x, gamma, row, G.C['gn_mean'], G.C['gn_var'])
        assert ok, (row, cls, wm, ws)
    x, gamma = K.stats_inputs(row, 0.0)
    N = HW * (Cc // groups)
    if N > 1:
        # (N = 262 160 elements per group: the unbiased variance moves rstd by 1 / (2 N) = 1.9e-6, inside the rule at c_gn = 64: not told there)
        for d in ('drop_last',) + (('unbiased',) if N < 100000 else ()):
            ok, wm, ws = K.stats_within(None, None, x, gamma, row, G.C['gn_mean'], G.C['gn_var'], defect=d)
            assert not ok, (row, d, wm, ws)
        x, gamma = K.stats_inputs(row, 'groups')
        ok, wm, ws = K.stats_within(None, None, x, gamma, row, G.C['gn_mean'], G.C['gn_var'], defect='no_eps')
        assert not ok, (row, 'no_eps', wm, ws)


def test_statistics_rule_documents_the_degradation():
    """the float32 restatement's rstd error grows with (mean / std)^2 as the rule says it may: the figures the header of groupnorm.hip and
    DESIGN.md quote (emulation on the CPU, not a GPU measurement)"""
    row = (128, 32, 255)
    for ratio in (10.0, 300.0, 1e4):
        x = K.normal((3 * 255, 128), 77, 1.0, ratio)
        mean, var, rstd = K.gn_ref(x, 3, 255, 128, 32)
        _, _, r2 = K.finalize_ref(K.gn_partials_f32(x, 3, 255, 128, 32), 255, 4)
        rel = float(((r2 - rstd).abs() / rstd).max())
        print(f'mean / std = {ratio:g}: restated rstd error {rel:.1e}, rule {float(K.rstd_bound(_G().C["gn_var"], mean, var).max()):.1e}')
        # (the rule is first order: at mean / std = 1e4 var cancels to nothing, rstd clamps at 1 / sqrt(eps) and is off by a factor)
        assert rel <= float(K.rstd_bound(_G().C['gn_var'], mean, var).max()) or ratio >= 1e4


@pytest.mark.parametrize('row', K.FIN_ROWS[::4] + K.FIN_ROWS[1::4] + K.FIN_ROWS[-4:], ids=_id)
def test_finalize_tolerance_tells_a_dropped_slot(row):
    n, ns, Cc, groups = row
    cg = Cc // groups
    part, gamma, HW = K.finalize_inputs(row)
    mean, var, rstd = K.finalize_ref(part, HW, cg)
    bm, br = K.finalize_bounds(part, HW, cg, ns)
    assert float(var[0, 0]) < 0 and float(rstd[0, 0]) == 1.0 / np.sqrt(K.EPS)
    assert K.within(mean.float(), mean, bm)[0] and K.within(rstd.float(), rstd, br * rstd)[0]
    if ns > 1:                                                     # (the count still the full one: mean and variance both move)
        dm, _, dr = K.finalize_ref(part, HW, cg, defect='drop_slot')
        assert not K.within(dm, mean, bm)[0] and K.within(dr[:, 1:], rstd[:, 1:], (br * rstd)[:, 1:])[1] > 1000


def test_apply_tolerance_tells_the_next_images_statistics():
    G = _G()
    for row in K.APPLY_ROWS:
        Cc, HW, n = row
        x, mc, sc, beta = K.apply_inputs(row)
        for sw in (False, True):
            ref, mag = K.apply_ref(x, mc, sc, beta, n, HW, Cc, sw)
            bound = K.apply_bound(G.C['apply'], ref, mag, sw)
            assert K.within(K.apply_ref(x, mc, sc, beta, n, HW, Cc, sw, dtype=torch.float32)[0], ref, bound)[0], (row, sw)
            assert not K.within(K.apply_ref(x, mc, sc, beta, n, HW, Cc, sw, defect='next_img')[0], ref, bound)[0], (row, sw)
            assert K.within(K.apply_ref(x, mc, sc, beta, n, HW, Cc, sw, defect='next_img')[0], ref, bound)[1] > 1000


@pytest.mark.parametrize('row', K.PRO_ROWS, ids=_id)
def test_prologue_tolerance_tells_a_wrong_image(row):
    """an image index taken one row early, and the first half-tile's image on rows 64 .. 127 of a tile (where the row's image differs):
    both at least 1000 x the f32 bound and 1000 x the standing 6e-7 of magnitude away"""
    G = _G()
    rpi = row[0]
    inp = K.pro_inputs(row)
    for sw in (False, True):
        ref, mag, MAG = K.pro_ref(row, inp, sw)
        bound = K.pro_bound(G.C['gemm_pro'], mag, MAG, sw, K.SWISH_U)
        assert K.within(K.pro_f32(row, inp, sw), ref, bound)[0], (row, sw)
        for d in K.PRO_DEFECTS:
            if d == 'half_prev' and rpi % 128 == 0:
                continue                                           # (no tile holds two images)
            bad, _, _ = K.pro_ref(row, inp, sw, defect=d)
            assert K.within(bad, ref, bound)[1] >= 1000, (row, sw, d)
            assert float(((bad - ref).abs() / mag).max()) >= 1000 * K.X6_MAX, (row, sw, d)
    M = rpi * row[1]
    assert (M % 128 == 0) == (row == K.PRO_ROWS[0])                # every other row ends in a clamped tile


@pytest.mark.parametrize('shape', K.ATTN_SHAPES, ids=_id)
def test_attention_tolerance_tells_the_defects(shape):
    G = _G()
    HW, Cc = shape
    n, scale, ld = 3, K.attn_scale(Cc), 3 * Cc + 8
    for cls in K.ATTN_CLASSES:
        q, k, v = K.attn_inputs(cls, HW, Cc, n)
        ref, M, S, p, _ = K.attn_ref(q, k, v, scale)
        bound = K.attn_bound(G.C['attn_pv'], G.C[K.attn_score_key(cls)], M, S)
        x3h = K.ATTN_X3H_ABS * max(1.0, float(ref.abs().max()))
        o32, _ = K.attn_f32(q, k, v, scale)
        assert K.within(o32, ref, bound)[0] if cls != 'exact' else K.mismatches(o32, ref) == 0, (shape, cls)
        qd, kd, vd = K.attn_unpack(torch.nan_to_num(K.attn_pack(q, k, v, ld), nan=3.0), n, HW, Cc, 3 * Cc)
        told = {'drop_tile': K.attn_ref(q, k, v, scale, defect='drop_tile')[0], 'no_scale': K.attn_ref(q, k, v, scale, defect='no_scale')[0],
                'ld': K.attn_ref(qd, kd, vd, scale)[0]}
        for d, bad in told.items():
            if (d, cls) in (('no_scale', 'exact'), ('no_scale', 'selector')):
                continue                                           # (q = 0 / a one-hot softmax: the scale does not reach the output)
            if cls == 'exact':
                assert K.mismatches(bad, ref) > 0, (shape, cls, d)
            else:
                assert not K.within(bad, ref, bound)[0], (shape, cls, d)
            assert float((bad - ref).abs().max()) > 100 * x3h, (shape, cls, d)
        if cls == 'exact':                                         # integer means scaled by 2^-8 / 2^-6, exact in fp32
            assert bool((ref * HW == (ref * HW).round()).all()) and bool((ref.float().double() == ref).all()) and HW in (64, 256)
        if cls == 'selector':                                      # the float64 reference's off-target mass
            perm = torch.from_numpy(K.attn_perm(HW))
            assert float((1 - p[:, torch.arange(HW), perm]).max()) < 2.0 ** -40
            assert K.ATTN_SELECT_A ** 2 * Cc ** 0.5 > 60 and float(q.abs().max()) == K.ATTN_SELECT_A
        if cls in K.ATTN_SHIFTS:
            _, _, _, _, s = K.attn_ref(q, k, v, scale)
            assert abs(float(s.mean()) - K.ATTN_SHIFTS[cls]) < 1.0 and float(q.abs().max()) < 64
            assert (float(s.min()) > 88.8) == (cls == 'shifted100')        # fp32 exp(s) overflows on every score of the + 100 class


def test_codebook_tolerances_tell_the_defects():
    G = _G()
    for D, Kc in K.CB_SHAPES:
        E = K.codebook(D, Kc)
        ref = E.double().pow(2).sum(0)
        assert K.worst_ratio(K.colsumsq_f32(E), ref, ref) <= G.C['colsumsq']
        assert K.worst_ratio(E[:-1].double().pow(2).sum(0), ref, ref) > 1000 * G.C['colsumsq']        # a dropped last row
        idx = K.gather_indices(Kc)
        assert K.mismatches(K.gather_ref(E, idx, defect='unclamped'), K.gather_ref(E, idx)) > 0
        assert torch.equal(K.gather_ref(E, idx)[3], E[:, 0]) and torch.equal(K.gather_ref(E, idx)[11], E[:, Kc - 1])
    z, E, want = K.tie_inputs()
    assert K.argmin_ref(z, E).tolist() == want and K.argmin_ref(z, E, defect='tie_high').tolist() != want
    assert K.argmin_ref(z, E, defect='tie_high').tolist() == [200, 130, 200, 256, 256, 72, 72, 130]


@pytest.mark.parametrize('row', K.CONV_IN_ROWS, ids=_id)
def test_conv_in_tolerance_tells_the_defects(row):
    G = _G()
    cout, n, H, W = row
    img, w, b = K.conv_in_inputs(row)
    for bias in (b, None):
        ref, mag = K.conv_in_ref(img, w, bias)
        assert K.worst_ratio(K.conv_in_f32(img, w, bias), ref, mag) <= G.C['conv_in']
        for d in ('div256', 'taps'):
            if d == 'taps' and (H == 1 and W == 1):
                continue                                           # (one pixel: only the centre tap is read)
            bad, _ = K.conv_in_ref(img, w, bias, defect=d)
            assert K.worst_ratio(bad, ref, mag) >= 1000 * G.C['conv_in'], (row, d)
            assert float(((bad - ref).abs() / mag).max()) >= 1000 * K.CONV_IN_X3H_MAX, (row, d)


@pytest.mark.parametrize('row', K.SMALL_ROWS, ids=_id)
def test_small_cout_tolerance_tells_the_defects(row):
    G = _G()
    x, w, b, mc, sc, beta = K.small_inputs(row, True)
    for pro in K.SMALL_PRO:
        p = None if pro is None else (mc, sc, beta)
        ref, mag, MAG = K.small_ref(x, w, b, p, pro == 'swish')
        bound = K.pro_bound(G.C['small'], mag, MAG, pro == 'swish', K.SWISH_1ULP_U)
        assert K.within(K.small_f32(x, w, b, p, pro == 'swish'), ref, bound)[0], (row, pro)
        for d in ('drop_chunk',) + (('pro_pad',) if pro else ()):
            assert K.within(K.small_ref(x, w, b, p, pro == 'swish', defect=d)[0], ref, bound)[1] >= 1000, (row, pro, d)
    xe, we, be = K.small_exact_inputs(row)
    ref, mag, _ = K.small_ref(xe, we, be, None, False)
    assert float(mag.max()) / 0.25 < CR.EXACT_HEADROOM and bool((ref.float().double() == ref).all())
    assert torch.equal(xe.to(torch.bfloat16).float(), xe) and K.mismatches(K.small_f32(xe, we, be, None, False), ref) == 0
    assert K.mismatches(K.small_ref(xe, we, be, None, False, defect='drop_chunk')[0], ref) > 0
    assert torch.equal(x.to(torch.bfloat16).float(), x)            # the bf16 class: values widened exactly


# ------------------------------------------------------------------ 4. the caps the GPU test leans on
@pytest.mark.parametrize('row', K.LOOKUP_ROWS, ids=_id)
def test_lookup_classes_stay_inside_their_caps(row):
    M, D, Kc = row
    z, E, k, dmin = K.planted_inputs(row)
    noise = (z.double() - E.double().t()[k]).norm(dim=1)
    assert float(noise.max()) <= 0.01 * dmin * (1 + 1e-4)
    d = K.dist64(z, E)
    two = d.topk(2, 1, largest=False).values
    assert torch.equal(d.argmin(1), k) and bool(((two[:, 1] - two[:, 0]) > 1000 * K.lookup_tau(z, E)).all())      # no exemption is needed
    ks = set(k.tolist())
    assert Kc - 1 in ks and (M < 4 or Kc <= 128 or {127, 128} <= ks)
    z, E = K.random_lookup_inputs(row)
    ok, share, msg = K.lookup_check(K.argmin_ref(z, E), z, E)
    assert ok and share <= 0.01, (row, share, msg)                 # by the reference's margins alone
    ok, _, _ = K.lookup_check((K.argmin_ref(z, E) + 1) % Kc, z, E)
    assert not ok


def test_tables_reach_the_forks_they_name():
    # statistics: lane counts 256 .. 1, HW below the lane count, split tails
    lanes = {256 // (Cc // 4) for Cc, _, _ in K.STATS_ROWS}
    assert lanes >= {256, 32, 8, 4, 2, 1} and any(HW < 256 // (Cc // 4) for Cc, _, HW in K.STATS_ROWS)
    assert K.gn_nsplit(513) == 2 and -(-513 // 2) == 257 and K.gn_nsplit(16385) == 64 and 16385 - 63 * -(-16385 // 64) < -(-16385 // 64)
    assert any(HW % K.gn_nsplit(HW) for _, _, HW in K.STATS_ROWS) and any(g == Cc for Cc, g, _ in K.STATS_ROWS) and any(g not in (32, Cc) for Cc, g, _ in K.STATS_ROWS)
    for Cc, g in K.STATS_REFUSED:
        assert Cc % 4 or (Cc // 4 > 256 or 256 % (Cc // 4)) or g > 256 or Cc % g
    # finalize: both kernels, the slot loop's tails, item counts off the 32- and 4-per-block grids
    assert {ns <= 512 for ns in K.FIN_SLOTS} == {True, False} and {ns % 8 for ns in K.FIN_SLOTS} >= {0, 1, 7} and {ns % 64 for ns in K.FIN_SLOTS} >= {0, 1, 63}
    assert {r[0] for r in K.FIN_ROWS} == set(K.FIN_N) and {r[2] for r in K.FIN_ROWS} == set(K.FIN_C)
    for big in (False, True):                                      # per kernel: an item count off its 32- resp. 4-per-block grid
        assert any((r[0] * r[3]) % (4 if big else 32) for r in K.FIN_ROWS if (r[1] > 512) == big)
    # apply: the second lap
    Cc, HW, n = K.APPLY_LAP
    assert n * HW * (Cc // 4) > 8192 * 256 and all(n_ * HW_ * (C_ // 4) <= 8192 * 256 for C_, HW_, n_ in K.APPLY_ROWS)
    # prologue: the three instantiations, the straddling tile, three column blocks
    assert {K.pro_form(r[0]) for r in K.PRO_ROWS} == {'img1', 'img2', 'generic'} and any(r[2] == 384 for r in K.PRO_ROWS)
    assert any(r[0] % 64 == 0 and r[0] % 128 and (r[0] // 64) % 2 == 1 and r[0] > 64 for r in K.PRO_ROWS)
    assert {r[1] for r in K.PRO_ROWS} == {3, 5} and {r[3] for r in K.PRO_ROWS} == {'full', 'no_bias', 'no_res'}
    # conv_in: CPT = 4 beside the Cout == 128 case, the laps, the LDS limit
    assert {r[0] for r in K.CONV_IN_ROWS} >= {4, 128, 256} and 28 * 1024 * 4 > 64 * 1024 >= 28 * 256 * 4
    (c0, n0, H0, W0), (c1, n1, H1, W1) = K.CONV_IN_LAPS
    assert c0 != 128 and n0 * H0 * W0 * (c0 // 4) > 8192 * 256 >= H0 * W0 * (c0 // 4)
    assert c1 == 128 and n1 * H1 * W1 * 8 > 16384 * 256 >= H1 * W1 * 8
    # conv3_small_cout: the largest accepted input and the first refused one
    assert max(r[0] for r in K.SMALL_ROWS) == 672 and 672 // 32 * 4608 == 96768 <= 96 * 1024 < 704 // 32 * 4608 and {r[1] for r in K.SMALL_ROWS} == {1, 2, 3, 4}
    # lookup: M = 1, 127, 128, 129, 385 against every codebook width
    assert {r[0] for r in K.LOOKUP_ROWS} == {1, 127, 128, 129, 385} and {r[2] for r in K.LOOKUP_ROWS} == {64, 200, 257, 1024} and {r[1] for r in K.LOOKUP_ROWS} == {32, 64, 256}
