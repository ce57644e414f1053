"""CPU: the float64 references of tests/gemm_kernels_ref.py pinned against independent statements (torch.nn.functional and its autograd for
the layer x @ W + b, its GELU and their gradients; a direct integer evaluation of the dropout hash), the comparison rules checked against
the ways these kernels go wrong, the tail policy and the dispatcher's restatement checked against the case tables, and the calibration
that the constants of tests/test_hip_gemm_kernels.py come from: the float32 restatement of every kernel class against float64 on the GPU
test's own inputs, in units of 2^-24 x magnitude."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_kernels_ref as G
import training_kernels_ref as R
import transformer_kernels_ref as X

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _same(a, b, tol=1e-12):
    a, b = R.t64(a), R.t64(b)
    return a.shape == b.shape and float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _covers(mag, val):
    return bool((R.t64(mag) >= R.t64(val).abs() * (1 - 1e-9)).all())


def _c(kernel):
    import test_hip_gemm_kernels as T
    return T.C[kernel]


def _pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


# ------------------------------------------------------------------ 1. pins
def test_bf16_rounding_against_its_integer_definition():
    """round to nearest even on the float32 pattern: add 0x7fff + the lowest kept bit, drop 16 bits; ties go both ways in the sample"""
    v = torch.cat((R.normal((4096,), 1), torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0, -0.0, 3.0e38])))     # 1 + 2^-8, 1 + 3 2^-8: ties
    bits = v.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    want = (((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16).to(torch.int64)
    want = torch.where(want >= 2 ** 31, want - 2 ** 32, want).to(torch.int32).view(F32).double()
    assert R.mismatches(G.bf16_rne(v), want) == 0
    assert float(G.bf16_rne(torch.tensor(1.00390625))) == 1.0 and float(G.bf16_rne(torch.tensor(1.01171875))) == 1.015625
    assert float(G.bf16_trunc(torch.tensor(1.0078))) == 1.0 and float(G.bf16_rne(torch.tensor(1.0078))) == 1.0078125
    assert float(G.bf16_rne(torch.tensor(G.SENTINEL))) == G.SENTINEL


@pytest.mark.parametrize('M,K,N', [(129, 64, 72), (255, 128, 130), (257, 384, 256)])
def test_forward_forms_against_functional_and_autograd(M, K, N):
    inp = G.forward_inputs(M, K, N, 'normal')
    x16, W16, b, res = inp['x'].to(BF16).double(), inp['W'].to(BF16).double(), inp['bias'].double(), inp['res'].double()
    pre0, mag0 = G.gemm(inp['x'], inp['W'])
    assert R.mismatches(pre0, G.gemm(inp['x'].to(BF16), inp['W'])[0]) == 0                  # x as it is stored = the rounding of float32 x
    lin = F.linear(x16, W16.t().contiguous(), b)
    w = G.wants('res', inp, pre0, mag0)['out']
    assert _same(w[0], lin + res) and _covers(w[1], w[0])
    w = G.wants('gelu_res', inp, pre0, mag0)['out']
    assert _same(w[0], F.gelu(lin) + res) and _covers(w[1], w[0])
    pre = lin.clone().requires_grad_(True)
    F.gelu(pre).sum().backward()
    w = G.wants('dual_grad', inp, pre0, mag0)
    assert _same(w['out'][0], pre.grad) and _same(w['aux'][0], F.gelu(lin)) and _covers(w['out'][1], w['out'][0])
    w = G.wants('dual', inp, pre0, mag0)
    assert _same(w['out'][0], lin) and _same(w['aux'][0], F.gelu(lin))
    for form, u in (('gelu_bwd', inp['u'].double()), ('gelu_bwd16', inp['u'].to(BF16).double())):
        uu = u.clone().requires_grad_(True)
        F.gelu(uu).backward(x16 @ W16)                                                     # the GELU backward with acc as the incoming gradient
        w = G.wants(form, inp, pre0, mag0)['out']
        assert _same(w[0], uu.grad) and _covers(w[1], w[0])
    w = G.wants('gelu_bwd16_grad', inp, pre0, mag0)['out']
    assert _same(w[0], (x16 @ W16) * inp['g16'].double())
    assert float(inp['u'].min()) == -12.0 and float(inp['u'].max()) == 12.0               # the sweep through GELU's tails is in u


def test_fast_erf_functions_against_the_row_kernels_restatements():
    """the GELU pieces of the bf16 arm restated here are X.gelu_bwd_fast_f32's (bit for bit through its bf16 result), and the erf
    approximation's own term covers the distance of the fast GELU from float64 where the erff form (X.gelu_f32) needs none"""
    u, df = X.gelu_inputs(1541)
    assert torch.equal((df * G.gelu_grad_fast_f32(u)).to(BF16), X.gelu_bwd_fast_f32(u, df))
    want, mag = X.gelu(u)
    term = 0.5 * u.double().abs() * G.FN_TERM
    erff, fast, fast_plain = R.worst_ratio(X.gelu_f32(u), want, mag), R.worst_ratio(G.gelu_fast_f32(u), want, mag + term), R.worst_ratio(G.gelu_fast_f32(u), want, mag)
    print(f'gelu on the sweep: erff form {erff:.2f}, fast form {fast:.2f} with the erf term in the magnitude, {fast_plain:.1f} without')
    assert erff < 4 and fast < 4 and fast_plain > 3 * fast
    d, dm = G.gelu_grad(u)
    assert R.worst_ratio(G.gelu_grad_fast_f32(u), d, dm + 0.5 * G.FN_TERM) < 4


def test_dropout_form_against_a_direct_evaluation_of_the_hash():
    """keep(m + row0, n) at hand-chosen elements from the integer definition (csrc/vf_common.h as viewformer_amd/_hash.py states it):
    word = lowbias32(group ^ hash(seed, site, 0)), group = ((m + row0) >> 2) N + n, keep = rotl32(word, 8 ((m + row0) & 3)) >= floor(rate 2^32)"""
    from viewformer_amd import _hash
    M, K, N, rate, row0 = 257, 128, 256, 0.1, 8
    key = int(_hash.dropout_hash(G.DROP_SEED, G.DROP_SITE, [0])[0])
    thresh = int(float(np.float32(rate)) * 4294967296.0)
    keep = G.drop_keep(np.arange(M), N, rate, G.DROP_SEED, G.DROP_SITE, row0)
    keep0 = G.drop_keep(np.arange(M), N, rate, G.DROP_SEED, G.DROP_SITE, 0)
    for m, n in ((0, 0), (1, 0), (3, 255), (4, 1), (130, 77), (255, 255), (256, 0), (256, 255)):
        g = ((m + row0) >> 2) * N + n
        word = int(_hash.lowbias32(np.asarray([g ^ key], dtype=np.uint64))[0])
        sh = 8 * ((m + row0) & 3)
        rot = ((word << sh) | (word >> (32 - sh))) & 0xFFFFFFFF if sh else word
        assert bool(keep[m, n]) == (rot >= thresh), (m, n)
    assert torch.equal(keep[:M - 8], keep0[8:])                                            # row0 shifts the mask by whole rows
    rows = np.arange(5, 605)                                                               # more than 2^17 elements: the whole-array evaluation
    g, sub = _hash.elem_group(np.broadcast_to((rows.astype(np.uint64) + np.uint64(row0))[:, None], (600, N)), np.arange(N, dtype=np.uint64)[None, :], N)
    direct = torch.from_numpy(np.ascontiguousarray(_hash.dropout_keep(G.DROP_SEED, G.DROP_SITE, g, sub, float(np.float32(rate)))))
    assert torch.equal(G.drop_keep(rows, N, rate, G.DROP_SEED, G.DROP_SITE, row0), direct)
    assert not torch.equal(keep, keep0) and 0.85 < float(keep.float().mean()) < 0.95
    inp = G.forward_inputs(M, K, N, 'normal')
    pre0, mag0 = G.gemm(inp['x'], inp['W'])
    w, m = G.wants('drop_res', inp, pre0, mag0, drop=(rate, row0))['out']
    lin = pre0 + inp['bias'].double()
    assert _same(w, inp['res'].double() + keep.double() * lin / (1.0 - float(np.float32(rate)))) and _covers(m, w)
    assert R.mismatches(w[~keep], inp['res'].double()[~keep]) == 0 and R.mismatches(m[~keep], inp['res'].double().abs()[~keep]) == 0
    # rate 0.5: the scale is exactly 2, the dyadic class stays exact
    inp = G.forward_inputs(M, K, N, 'dyadic')
    pre0, mag0 = G.gemm(inp['x'], inp['W'])
    w, _ = G.wants('drop_res', inp, pre0, mag0, drop=(0.5, row0))['out']
    assert R.mismatches(G.restated('drop_res', inp, G.gemm_f32(inp['x'], inp['W']), drop=(0.5, row0))['out'], w) == 0


@pytest.mark.parametrize('M,K,N,splits', G.TN_CASES)
def test_weight_gradient_against_autograd(M, K, N, splits):
    for y16 in (False, True):
        x16, dy = G.tn_inputs(M, K, N, 'normal')
        dy = dy.to(BF16) if y16 else dy
        W = torch.zeros((K, N), dtype=F64, requires_grad=True)
        b = torch.zeros(N, dtype=F64, requires_grad=True)
        y = x16.double() @ W
        y.backward(dy.to(BF16).double())                                                   # the product takes the rounded dy
        (y.detach() + b).backward(dy.double())                                             # the bias gradient takes dy as it is stored
        dW, mW, db, mb = G.gemm_tn(x16, dy, splits)
        assert _same(dW.sum(0), W.grad) and _same(db.sum(0), b.grad) and _covers(mW, dW) and _covers(mb, db)
        chunks = G.tn_chunks(M, splits)
        assert chunks[0][0] == 0 and chunks[-1][1] == M // 64 and all(a[1] == b_[0] for a, b_ in zip(chunks, chunks[1:]))
        assert all(c1 > c0 for c0, c1 in chunks)
    assert G.tn_chunks(320, 3) == [(0, 1), (1, 3), (3, 5)] and G.tn_chunks(320, 5) == [(i, i + 1) for i in range(5)]


def test_selector_inputs_select():
    x, pi = G.selector(192, 5)
    W = R.normal((192, 72), 6, 0.05)
    assert R.mismatches(G.gemm(x, W)[0], G.bf16_rne(W)[pi]) == 0 and sorted(pi.tolist()) == list(range(192))
    x16, dy = G.tn_inputs(256, 256, 256, 'normal')
    xs, pi = G.selector(256, 7)
    dW = G.gemm_tn(xs.to(BF16), dy, 4)[0]
    assert R.mismatches(dW.sum(0)[pi], G.bf16_rne(dy)) == 0
    assert R.mismatches(dW[1][pi[64:128]], G.bf16_rne(dy)[64:128]) == 0 and float(dW[1][pi[:64]].abs().max()) == 0.0


def test_dyadic_inputs_are_exact_in_float32_in_any_order():
    for M, K, N in ((129, 192, 72), (640, 384, 256)):
        inp = G.forward_inputs(M, K, N, 'dyadic')
        assert R.mismatches(G.bf16_rne(inp['W']), inp['W']) == 0 and float(inp['x'].abs().max()) <= 8
        pre0, mag0 = G.gemm(inp['x'], inp['W'])
        acc = G.gemm_f32(inp['x'], inp['W'])
        assert R.mismatches(acc, pre0) == 0
        back = torch.zeros_like(acc)
        for k in reversed(range(0, K, 16)):
            back = back + inp['x'][:, k:k + 16] @ inp['W'][k:k + 16]
        assert R.mismatches(back, pre0) == 0
        for form in ('res', 'dual', 'gelu_bwd16_grad'):
            w, got = G.wants(form, inp, pre0, mag0), G.restated(form, inp, acc)
            assert R.mismatches(got['out'], w['out'][0]) == 0, form
    x16, dy = G.tn_inputs(320, 256, 256, 'dyadic')
    dW, _, db, _ = G.gemm_tn(x16, dy, 3)
    gW, gb = G.gemm_tn_f32(x16, dy, 3)
    assert R.mismatches(gW, dW) == 0 and R.mismatches(gb, db) == 0


# ------------------------------------------------------------------ 2. the tables reach what they are listed under
def test_tail_policy_returns_the_tuples_of_the_case_table():
    for M, tup in G.TAIL_CASES:
        assert G.tail_policy(M, G.TAIL_N) == tup, M
        assert G.tail_policy(M, G.TAIL_N, tail_on=False) is None
        f, h, ic = tup
        assert f * 256 + h * 64 * ic >= M > f * 256 + (h - 1) * 64 * ic                    # the tail tiles cover the rows, the last one is not empty
        rows = G.tail_rows(M, tup)
        assert int(rows[0]) == 0 and int(rows[-1]) == M - 1 and rows.numel() == 512 + M - f * 256
    assert (4282 - 4096) % 128 == 58 and (6196 - 4096) % 192 == 180                        # ragged 128-row and 192-row tail tiles
    for M in G.G256_M:
        for N in G.G256_N:
            assert G.tail_policy(M, N) is None                                             # one round: the plain grid
    # the workload's own shapes (tests/test_hip_bf16.py): the training step's 19200 rows take the policy at 3072 columns
    assert G.tail_policy(19200, 3072) is not None and G.tail_policy(256, 256) is None


def test_every_listed_shape_reaches_its_kernel():
    for K in G.STAGED_K:
        for M in G.STAGED_M:
            for N in G.STAGED_N:
                for form in G.STAGED_FORMS:
                    assert G.forward_kernel(M, K, N, False, False, form) == 'staged'
    for M, N in G.STAGED_BATCHED:
        assert G.forward_kernel(M, 64, N, False, False, 'none', batch=3, lda=192) == 'staged'
    assert G.forward_kernel(129, 128, 72, False, False, 'none', batch=3) == 'staged'       # a batch keeps K % 128 == 0 on the staged kernel
    for K in G.DIRECT_K:
        for M, N in G.DIRECT_MN:
            for a16 in (False, True):
                for o16 in (False, True):
                    for form in G.DIRECT_FORMS[o16]:
                        for ldc in G.direct_ldc(N):
                            assert G.forward_kernel(M, K, N, a16, o16, form, ldc=ldc) == 'direct', (M, K, N, a16, o16, form)
    for M in G.G256_M:
        for K in G.G256_K:
            for N in G.G256_N:
                for o16 in (False, True):
                    for form in G.G256_FORMS[o16]:
                        for pa, pc, pr, pr16 in G.G256_PADS:
                            ldr = N + (pr16 if G.FORMS[form].get('res16') else pr)
                            assert G.forward_kernel(M, K, N, True, o16, form, lda=K + pa, ldc=N + pc, ldr=ldr) == 'g256'
                for rate, row0, form in G.G256_DROPS:
                    assert G.forward_kernel(M, K, N, True, False, form, row0=row0) == 'g256'
    M, K, N = G.G256_BOTH
    assert G.forward_kernel(M, K, N, True, False, 'res', g256_on=False) == 'direct'
    assert G.forward_kernel(M, K, N, True, True, 'gelu', g256_on=False) == 'direct'
    assert G.forward_kernel(M, K, N, True, False, 'gelu_res') == 'direct'                  # the one form of 256-tile shapes the 128-tile kernel keeps
    for M, _ in G.TAIL_CASES:
        for form, o16 in G.TAIL_FORMS:
            assert G.forward_kernel(M, G.TAIL_K, G.TAIL_N, True, o16, form, row0=G.TAIL_DROP[1]) == 'g256'
    for M, K, N, splits in G.TN_CASES:
        assert K % 256 == 0 and N % 256 == 0 and M % 64 == 0 and splits <= M // 64
    assert sorted({(K // 256) * (N // 256) * s for M, K, N, s in G.TN_CASES}) == [1, 3, 5, 6]
    assert G.SLAB_N[-1] == 4 * (4096 * 256 + 1)


def test_the_refusals_of_the_restated_dispatcher():
    B, Un = G.BAD_ARG, G.UNSUPPORTED
    fk = G.forward_kernel
    assert fk(128, 96, 128, False, False, 'none') == Un                                    # K % 64
    assert fk(128, 128, 128, False, False, 'none', lda=124) == B and fk(128, 128, 128, False, False, 'none', lda=130) == B
    assert fk(128, 128, 128, True, False, 'none', lda=132) == B                            # bf16 x: lda & 7
    assert fk(128, 128, 128, False, True, 'res') == B and fk(256, 128, 256, True, True, 'res') == B
    assert fk(256, 128, 256, True, False, 'gelu_bwd') == Un
    assert fk(256, 128, 256, True, False, 'bias', aux=True) == B and fk(256, 128, 256, True, False, 'dual', aux=False) == B
    for form in ('dual', 'drop'):
        assert fk(255, 128, 256, True, False, form) == Un and fk(256, 128, 128, True, False, form) == Un
    assert fk(256, 192, 256, True, False, 'bias') == Un and fk(256, 192, 256, False, True, 'bias') == Un


# ------------------------------------------------------------------ 3. the rules reject wrong kernels
def _fwd(M, K, N, cls='normal'):
    inp = G.forward_inputs(M, K, N, cls)
    pre0, mag0 = G.gemm(inp['x'], inp['W'])
    return inp, pre0, mag0, G.gemm_f32(inp['x'], inp['W'])


def _rejected32(got, want, mag, c):
    """elements the float32 rule rejects"""
    got, want, mag = R.t64(got), R.t64(want), R.t64(mag)
    return int((~((got - want).abs() <= c * R.U * mag)).sum())


def test_rejects_a_lost_k_step_a_neighbours_bias_and_a_clamped_residual_row():
    M, K, N = 300, 192, 200
    inp, pre0, mag0, acc0 = _fwd(M, K, N)
    c = _c('staged')
    want, mag = G.wants('res', inp, pre0, mag0)['out']
    good = G.restated('res', inp, acc0)['out']
    assert _rejected32(good, want, mag, c) == 0
    # one 16-deep step lost in the ragged corner tile (rows 256 .., columns 128 ..)
    lost = G.gemm_f32(inp['x'], inp['W'], lost=(256, 300, 128, 200, 64))
    bad = G.restated('res', inp, lost)['out']
    n = _rejected32(bad, want, mag, c)
    assert R.rejects(bad, want, mag, c) and n > 0.99 * 44 * 72 and _rejected32(bad[:256], want[:256], mag[:256], c) == 0
    # the bias of column n + 1 in the last column block
    b1 = inp['bias'].clone()
    b1[128:199] = inp['bias'][129:200]
    bad = acc0 + b1 + inp['res']
    assert _rejected32(bad, want, mag, c) > 0.9 * M * 71 and _rejected32(bad[:, :128], want[:, :128], mag[:, :128], c) == 0
    # the residual's row clamped to the tile's first row in the ragged last row tile
    r1 = inp['res'].clone()
    r1[256:] = inp['res'][256]
    bad = (acc0 + inp['bias']) + r1
    assert _rejected32(bad, want, mag, c) > 0.9 * 43 * N and _rejected32(bad[:257], want[:257], mag[:257], c) == 0


def test_rejects_truncation_on_the_bf16_store_and_of_x():
    M, K, N = 255, 128, 130
    inp, pre0, mag0, acc0 = _fwd(M, K, N)
    c = _c('direct')
    want, mag = G.wants('bias', inp, pre0, mag0)['out']
    good = G.restated('bias', inp, acc0)['out']
    assert G.interval_violations(good.to(BF16), want, G.bound(mag, c)) == 0
    n_trunc = G.interval_violations(G.bf16_trunc(good), want, G.bound(mag, c))
    assert n_trunc > 0.3 * M * N                                                          # truncation: wrong whenever the dropped bits exceed a half
    # a relative 2^-8 allowance lets most of them through (a bf16 ulp is 2^-8 .. 2^-7 of the value): what the interval rule is for
    n_rel = int((~((G.bf16_trunc(good) - want).abs() <= 2.0 ** -8 * want.abs() + G.bound(mag, c))).sum())
    assert n_rel < 0.6 * n_trunc
    # x truncated to bf16 instead of rounded
    xt = G.bf16_trunc(inp['x']).float()
    bad = G.gemm_f32(xt, inp['W']) + inp['bias']
    assert float((G.bf16_trunc(inp['x']) - G.bf16_rne(inp['x'])).abs().max()) > 0
    assert _rejected32(good, want, mag, c) == 0 and _rejected32(bad, want, mag, c) > 0.99 * M * N


def test_rejects_gelu_for_its_derivative_and_a_dual_gelu_of_the_rounded_value():
    M, K, N = 257, 128, 256
    inp, pre0, mag0, acc0 = _fwd(M, K, N)
    for form in ('gelu_bwd', 'gelu_bwd16'):
        c = _c('g256 gelu_bwd')
        want, mag = G.wants(form, inp, pre0, mag0)['out']
        good = G.restated(form, inp, acc0)['out']
        assert G.interval_violations(good.to(BF16), want, G.bound(mag, c)) == 0
        u = inp['u'].to(BF16).float() if form == 'gelu_bwd16' else inp['u']
        bad = acc0 * G.gelu_fast_f32(u)
        assert G.interval_violations(bad.to(BF16), want, G.bound(mag, c)) > 0.9 * M * N
        # a derivative wrong in the negative tail only: gelu'(u) = 0 below -3
        tail = acc0 * torch.where(u < -3.0, torch.zeros_like(u), G.gelu_grad_fast_f32(u))
        n = G.interval_violations(tail.to(BF16), want, G.bound(mag, c))
        assert 0 < n <= int((u < -3.0).sum())
    c = _c('g256 gelu')
    w = G.wants('dual', inp, pre0, mag0)
    got = G.restated('dual', inp, acc0)
    assert G.interval_violations(got['aux'].to(BF16), w['aux'][0], G.bound(w['aux'][1], c)) == 0
    assert G.interval_violations(got['out'].to(BF16), w['out'][0], G.bound(w['out'][1], _c('g256'))) == 0
    bad = G.gelu_fast_f32(got['out'].to(BF16).float())                                    # the GELU of the rounded pre-activation
    assert G.interval_violations(bad.to(BF16), w['aux'][0], G.bound(w['aux'][1], c)) > 0.05 * M * N
    w = G.wants('dual_grad', inp, pre0, mag0)
    got = G.restated('dual_grad', inp, acc0)
    assert G.interval_violations(got['out'].to(BF16), w['out'][0], G.bound(w['out'][1], _c('g256 gelu_grad'))) == 0
    assert G.interval_violations(got['aux'].to(BF16), w['out'][0], G.bound(w['out'][1], _c('g256 gelu_grad'))) > 0.9 * M * N      # gelu where gelu' belongs


def test_rejects_dropout_without_row0_and_after_the_residual():
    M, K, N, rate, row0 = 257, 128, 256, 0.1, 8
    inp, pre0, mag0, acc0 = _fwd(M, K, N)
    c = _c('g256 drop')
    want, mag = G.wants('drop_res', inp, pre0, mag0, drop=(rate, row0))['out']
    good = G.restated('drop_res', inp, acc0, drop=(rate, row0))['out']
    assert _rejected32(good, want, mag, c) == 0
    bad = G.restated('drop_res', inp, acc0, drop=(rate, 0))['out']                         # row0 ignored
    assert _rejected32(bad, want, mag, c) > 0.1 * M * N
    keep = G.drop_keep(np.arange(M), N, rate, G.DROP_SEED, G.DROP_SITE, row0)
    scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(rate))
    late = torch.where(keep, ((acc0 + inp['bias']) + inp['res']) * scale, torch.zeros(()))  # the mask applied after the residual joined
    assert _rejected32(late, want, mag, c) > 0.9 * M * N
    unscaled = torch.where(keep, acc0 + inp['bias'], torch.zeros(())) + inp['res']
    assert _rejected32(unscaled, want, mag, c) > 0.8 * M * N


def test_rejects_wrong_weight_gradients():
    M, K, N, splits = 320, 256, 256, 3
    x16, dy = G.tn_inputs(M, K, N, 'normal')
    cW, cb = _c('tn dW'), _c('tn db')
    dW, mW, db, mb = G.gemm_tn(x16, dy, splits)
    gW, gb = G.gemm_tn_f32(x16, dy, splits)
    assert _rejected32(gW, dW, mW, cW) == 0 and _rejected32(gb, db, mb, cb) == 0
    bW, _ = G.gemm_tn_f32(x16, dy, splits, unrounded_dy=True)                               # products with the unrounded dy
    assert _rejected32(bW, dW, mW, cW) > 0.9 * splits * K * N
    _, bb = G.gemm_tn_f32(x16, dy, splits, db_rounded=True)                                # db from the rounded dy where dy is float32
    assert _rejected32(bb, db, mb, cb) > 0.5 * splits * N
    # ... which is the reference when dy arrives as bf16
    d16 = G.gemm_tn(x16, dy.to(BF16), splits)
    assert _rejected32(bb, d16[2], d16[3], cb) == 0 and _rejected32(gW, d16[0], d16[1], cW) == 0
    sW, smW, sb, smb = G.gemm_tn(x16, dy, splits, shift=1)                                 # every split's chunk range moved by one chunk
    assert _rejected32(sW, dW, mW, cW) > 0.9 * splits * K * N and _rejected32(sb, db, mb, cb) > 0.9 * splits * N
    # the fold of a correct set of slabs meets the folded reference
    fw, fm = G.fold(dW, mW)
    assert _rejected32(G.fold_f32(gW), fw, fm, cW) == 0


def test_the_fold_in_reverse_order_differs_in_its_bits():
    for nslabs in (7, 9, 17):
        slabs = R.normal((nslabs, 1028), 40 + nslabs) * torch.logspace(0, 3, nslabs).view(-1, 1)   # growing slabs: the order shows
        dst0 = R.normal((1028,), 41)
        for d in (None, dst0):
            a, b = G.fold_f32(slabs, d), G.fold_f32(slabs, d, reverse=True)
            assert int((a.view(torch.int32) != b.view(torch.int32)).sum()) > 100
            w, m = G.fold(slabs.double(), slabs.double().abs(), d)
            assert R.worst_ratio(a, w, m) < nslabs                                         # ... while both are sums of the same numbers
    assert R.mismatches(G.fold_f32(R.normal((1, 8), 1)), R.normal((1, 8), 1)[0]) == 0


# ------------------------------------------------------------------ 4. calibration
def _note(cal, key, got, want_mag):
    cal[key] = max(cal.get(key, 0.0), R.worst_ratio(got, *want_mag))


def _forward_cal(cal, kernel, M, K, N, forms, rows=None, drops=((0.1, 8),)):
    inp = G.forward_inputs(M, K, N, 'normal', saved=rows is None)
    x = inp['x'] if rows is None else inp['x'][rows]
    pre0, mag0 = G.gemm(x, inp['W'])
    acc0 = G.gemm_f32(x, inp['W'])
    for form in forms:
        for drop in (drops if G.FORMS[form].get('drop') else (None,)):
            w, got = G.wants(form, inp, pre0, mag0, rows, drop), G.restated(form, inp, acc0, rows, drop)
            for name in w:
                fn = G.fn_class(form, name)
                _note(cal, kernel + (' ' + fn if fn else ''), got[name], w[name])


def calibration():
    """the worst distance of each kernel class's float32 restatement from float64 over the GPU test's normal-class inputs"""
    cal = {}
    for K in G.STAGED_K:
        for M in G.STAGED_M:
            for N in G.STAGED_N:
                _forward_cal(cal, 'staged', M, K, N, G.STAGED_FORMS)
    for M, N in G.STAGED_BATCHED:
        inp = G.forward_inputs(M, 192, N, 'normal')
        dst0 = inp['res']
        parts = G.splitk(inp['x'], inp['W'], 3)
        _note(cal, 'splitk', G.splitk_f32(inp['x'], inp['W'], 3, dst0), G.fold([p[0] for p in parts], [p[1] for p in parts], dst0))
    for K in G.DIRECT_K:
        for M, N in G.DIRECT_MN:
            _forward_cal(cal, 'direct', M, K, N, sorted(set(G.DIRECT_FORMS[False] + G.DIRECT_FORMS[True])))
    for M in G.G256_M:
        for K in G.G256_K:
            for N in G.G256_N:
                _forward_cal(cal, 'g256', M, K, N, sorted(set(G.G256_FORMS[False] + G.G256_FORMS[True])) + ['drop', 'drop_res'], drops=((0.1, 0), (0.1, 8)))
    for M, tup in G.TAIL_CASES:
        _forward_cal(cal, 'tail', M, G.TAIL_K, G.TAIL_N, [f for f, _ in G.TAIL_FORMS], rows=G.tail_rows(M, tup), drops=(G.TAIL_DROP,))
    for M, K, N, splits in G.TN_CASES:
        x16, dy = G.tn_inputs(M, K, N, 'normal')
        for y in (dy, dy.to(BF16)):
            dW, mW, db, mb = G.gemm_tn(x16, y, splits)
            gW, gb = G.gemm_tn_f32(x16, y, splits)
            _note(cal, 'tn dW', gW, (dW, mW))
            _note(cal, 'tn db', gb, (db, mb))
            dst0 = R.normal((K, N), 77)
            _note(cal, 'tn dW', G.fold_f32(gW, dst0), G.fold(dW, mW, dst0))
            _note(cal, 'tn db', G.fold_f32(gb), G.fold(db, mb))
    return cal


def test_calibration_covers_the_gpu_tests_constants():
    """c = 4 x the float32 restatement's worst error, rounded up to a power of two; the basis recorded beside it in the GPU test's table is
    within a binade of this run's, and four times this run's figure stays below the table's c (a changed input cannot silently loosen a
    constant).  A restatement's 16-deep sums depend on how torch's matmul orders them, hence no tighter pin of the basis itself"""
    import test_hip_gemm_kernels as T
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        cal = calibration()
    finally:
        torch.set_num_threads(threads)
    for k in sorted(cal):
        print(f'{k:18s} basis {cal[k]:7.3f} x 2^-24 x magnitude -> c = {_pow2_ceil(4 * cal[k]):g}   (table: basis {T.BASIS.get(k, 0):g}, c = {T.C.get(k, 0):g})')
    assert set(cal) == set(T.C) == set(T.BASIS)
    for k, v in cal.items():
        assert T.C[k] == _pow2_ceil(4 * T.BASIS[k]), k
        assert 4 * v <= T.C[k] and v <= 2 * T.BASIS[k] and T.BASIS[k] <= 2 * v, (k, v, T.BASIS[k], T.C[k])
