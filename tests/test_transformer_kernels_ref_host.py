"""CPU: the float64 references of tests/transformer_kernels_ref.py pinned against independent statements (torch.nn.functional and its
autograd, oracle/migt_oracle.py for the view masks, oracle/train_oracle.py for the AdamWeightDecay step, oracle/vqgan_oracle.py for the
uint8 post-process), the comparison checked against the ways these kernels go wrong, and the calibration that the constants of
tests/test_hip_transformer_kernels.py come from: a float32 CPU restatement of every rounded kernel against float64 on the GPU test's own
inputs, in units of 2^-24 x magnitude."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import training_kernels_ref as R
import transformer_kernels_ref as X

F64 = torch.float64


def _same(a, b, tol=1e-12):
    a, b = R.t64(a), R.t64(b)
    return a.shape == b.shape and float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _covers(mag, val):
    return bool((R.t64(mag) >= R.t64(val).abs() * (1 - 1e-9)).all())


# ------------------------------------------------------------------ 1. pins
def test_exact_class_against_torch_and_numpy():
    for rows, cols in X.TRANSPOSE_SHAPES:
        for batch, (ps, _), bf16 in X.TRANSPOSE_VARIANTS:
            src = X.transpose_input(rows, cols, batch, ps, bf16)
            assert R.mismatches(X.transpose(src, rows, cols)[0], src.double()[:, :, :cols].permute(0, 2, 1)) == 0
    for BS, L, d, V in X.EMBED_CASES:
        ids, wte, wpe, add = X.embed_inputs(BS, L, d, V)
        assert int(ids.min()) == 0 and int(ids.max()) == V - 1
        want = F.embedding(ids.long(), wte.double()) + wpe.double() + add.double()[:, None]
        got, _ = X.embed_sum(ids, wte, wpe, add, BS, L, d)
        assert R.mismatches(got, want.reshape(BS * L, d)) == 0
        assert R.mismatches(((wte[ids.long()] + wpe) + add[:, None]).reshape(BS * L, d), got) == 0          # exact in float32 too
    for n in X.ARGMAX_N:
        for rows in (1, 5):
            for kind in X.ARGMAX_KINDS:
                x = X.argmax_input(rows, n, kind)
                got, _ = X.argmax_rows(x, n)
                assert R.mismatches(got, np.argmax(x.numpy()[:, :n], axis=1)) == 0, (n, rows, kind)
                if kind in ('all_equal', 'all_neg_inf'):
                    assert int(got.abs().max()) == 0


def test_postprocess_against_the_oracle():
    from oracle import vqgan_oracle as vq
    x = X.postprocess_input()
    assert x.numel() == 255 * 5 + 6
    want = vq.postprocess_u8(x.view(1, 1, 1, -1)).reshape(-1)
    got, _ = X.postprocess_u8(x)
    assert R.mismatches(got, want) == 0
    # the float32 operations move a step up to a few ulps below x_k: the value two above it is always past the step, the value two below
    # it is before the step for most k
    steps, k = want[:255 * 5].view(255, 5).int(), torch.arange(1, 256)
    assert bool((steps[:, -1] == k).all()) and bool((steps[:, 0] >= k - 1).all()) and int((steps[:, 0] == k - 1).sum()) > 128
    assert want[-6:].tolist() == [0, 0, 127, 127, 255, 255]


@pytest.mark.parametrize('rows,d', [(5, 4), (5, 260), (1, 1024), (5, 2048)])
def test_layernorm_against_functional(rows, d):
    x, gamma, beta = X.ln_inputs(rows, d)
    v, m = X.layernorm(x, gamma, beta, X.LN_EPS)
    assert _same(v, F.layer_norm(x.double(), (d,), gamma.double(), beta.double(), eps=X.LN_EPS), 1e-10) and _covers(m, v)
    if rows == 5:
        assert float(x[1].std()) == 0.0 and abs(float(x[2].mean()) - 100.0) < 0.01


@pytest.mark.parametrize('rows,d', [(37, 4), (37, 260), (17, 260), (37, 768)])
def test_layernorm_backward_against_autograd(rows, d):
    dy, x, gamma, res, dg0, db0 = X.ln_bwd_inputs(rows, d)
    xx, g = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    b = torch.zeros(d, dtype=F64, requires_grad=True)
    F.layer_norm(xx, (d,), g, b, eps=X.LN_EPS).backward(dy.double())
    (dx, dg, db), mags = X.layernorm_bwd(dy, x, gamma, X.LN_EPS)
    assert _same(dx, xx.grad, 1e-10) and _same(dg, g.grad, 1e-10) and _same(db, b.grad, 1e-10)
    assert all(_covers(m, v) for m, v in zip(mags, (dx, dg, db)))
    (ax, ag, ab), mags = X.layernorm_bwd(dy, x, gamma, X.LN_EPS, res, dg0, db0)
    assert _same(ax, xx.grad + res.double(), 1e-10) and _same(ag, dg0.double() + g.grad, 1e-10) and _same(ab, db0.double() + b.grad, 1e-10)
    assert all(_covers(m, v) for m, v in zip(mags, (ax, ag, ab)))


def test_gelu_against_functional():
    u, df = X.gelu_inputs(1541)
    assert sorted(u.tolist()) == sorted(X.gelu_sweep().tolist()) and float(X.gelu_inputs(1)[0][0]) == -1.0625
    uu = u.double().requires_grad_(True)
    y = F.gelu(uu)
    y.backward(df.double())
    v, m = X.gelu(u)
    assert _same(v, y.detach()) and _covers(m, v)
    v, m = X.gelu_bwd(u, df)
    assert _same(v, uu.grad) and _covers(m, v)
    fast = X.gelu_bwd_fast_f32(u, df)
    assert fast.dtype == torch.bfloat16 and R.worst_ratio(fast.float(), v, X.gelu_bwd_bf16_bound(v, df)) < 4.0


def test_softmax_and_cross_entropy_against_functional():
    x = X.softmax_logits(5, 65)
    p, m = X.softmax_rows(x, 0.0625)
    assert _same(p, F.log_softmax(x.double() * 0.0625, -1).exp()) and _covers(m, p)
    for rows, V, spread in ((5, 65, False), (1, 1, False), X.CE_SPREAD + (True,)):
        logits, t, w = X.ce_inputs(rows, V, spread)
        assert int(t[0]) == 0 and int(t[-1]) == V - 1 and (rows < 3 or float(w[2]) == 0.0)
        assert not spread or float(logits.max()) > 59.0 and float(logits.min()) < -59.0
        for eps in X.CE_SMOOTHING:
            e = X.f32(eps)
            xx = logits.double().requires_grad_(True)
            loss = F.cross_entropy(xx, t.long(), reduction='none', label_smoothing=e)
            (loss * w.double()).sum().backward()
            (l, dl), (ml, mdl) = X.softmax_ce(logits, t, w, e)
            assert _same(l, loss.detach(), 1e-10) and _same(dl, xx.grad, 1e-10) and _covers(ml, l) and _covers(mdl, dl)


def _oracle_probabilities(s, T, L, spec):
    """the attention weights oracle/migt_oracle.py forms for scores ``s`` [T][T] under a mask spec: queries = the score rows and keys = values =
    rows of the identity make q k^T the scores and w v the weights.  Plain: compute_causal_block_attention over all views.  Streams of Sv
    views: compute_causal_block_multiend_attention, the first stream its main sequence, every later stream a branch of Sv views.  Twin
    views from Vc on: views below Vc are block-causal among themselves; view Vc is the one query view of a main sequence 0 .. Vc (its
    last view) and every later view a branch of one view.  A last view that is not full is filled
    up with keys of score -1e300 (weight 0 wherever they are visible) and queries that are dropped again"""
    from oracle import migt_oracle as mg
    nv = (T + L - 1) // L
    Tp = nv * L
    sp = torch.full((Tp, Tp), -1e300, dtype=F64)
    sp[:, :T] = 0.0
    sp[:T, :T] = s
    eye = torch.eye(Tp, dtype=F64)
    def pick(t, views):
        return torch.cat([t[v * L:(v + 1) * L] for v in views]).view(1, 1, len(views), L, Tp)

    def plain(views):
        return mg.compute_causal_block_attention(pick(eye, views), pick(eye, views), pick(sp, views))
    if spec == -1:
        out = [plain(list(range(nv)))]
    elif spec <= -2:
        ks = [pick(eye, list(range(i, i - spec))) for i in range(0, nv, -spec)]
        out = mg.compute_causal_block_multiend_attention(ks, ks, [pick(sp, list(range(i, i - spec))) for i in range(0, nv, -spec)])
    else:
        ks = [pick(eye, list(range(spec + 1)))] + [pick(eye, [v]) for v in range(spec + 1, nv)]
        out = [plain(list(range(spec)))] + mg.compute_causal_block_multiend_attention(ks, ks, [pick(sp, [v]) for v in range(spec, nv)])
    return torch.cat([o.reshape(-1, Tp) for o in out])[:T, :T]


@pytest.mark.parametrize('case', X.MASK_CASES)
def test_masks_against_the_oracle(case):
    batch, T, L, spec, scale = case
    s, dp = X.mask_inputs(batch, T, L, spec)
    p, m = X.softmax_mask(s, T, L, spec, scale)
    vis = X.visible(T, L, spec)
    assert bool((p[:, ~vis] == 0).all()) and bool((m[:, ~vis] == 0).all()) and bool((p[:, vis] > 0).all()) and _covers(m, p)
    assert bool(vis.diagonal().all())
    for b in range(batch):
        want = torch.softmax(s[b].double() * scale, -1) if L == 0 else _oracle_probabilities(s[b].double() * scale, T, L, spec)
        assert _same(p[b], want), case
    # the backward: autograd through the reference's own masking expression
    ss = s.double().requires_grad_(True)
    mk = vis.double()
    torch.softmax((ss * scale) * mk - 1e4 * (1 - mk), -1).backward(dp.double())
    ds, mds = X.softmax_mask_bwd(p, dp, T, L, spec, scale)
    assert _same(ds, ss.grad, 1e-10) and _covers(mds, ds) and bool((ds[:, ~vis] == 0).all())


def test_adamw_against_the_oracle():
    from oracle import train_oracle as to
    from viewformer_amd.config import MIGTConfig
    cfg = MIGTConfig(learning_rate=1e-3, weight_decay=0.05, total_steps=100)
    n = 1027
    p0, g0, m0, v0 = (t.double() for t in X.adamw_inputs(n))
    names = ('a.weight', 'a.bias')
    cut = {'a.weight': slice(0, 1000), 'a.bias': slice(1000, n)}
    mask = X.nodecay_mask(n, [(1000, n)])                                      # the oracle skips the decay of a name holding "bias"
    # (beta = 0.5 and 0.75: 1 - beta formed from the float32 beta is the oracle's float64 1 - beta, so the two agree to float64 rounding)
    b1, b2 = 0.5, 0.75
    p, g, m, v = ({k: t[cut[k]].numpy().copy() for k in names} for t in (p0, g0, m0, v0))
    lr = to.adam_weight_decay_step(p, g, m, v, step=5, cfg=cfg, warmup_steps=10, b1=b1, b2=b2, eps=1e-8)
    lr_t = lr * math.sqrt(1 - b2 ** 6) / (1 - b1 ** 6)
    (w, m1, v1), mags = X.adamw(p0, g0, m0, v0, lr * cfg.weight_decay, lr_t, b1, b2, 1e-8, nodecay=mask)
    for got, want in ((w, p), (m1, m), (v1, v)):
        assert _same(got, np.concatenate([want[k] for k in names]), 1e-13)
    assert all(_covers(mm, vv) for mm, vv in zip(mags, (w, m1, v1)))
    assert not _same(X.adamw(p0, g0, m0, v0, lr * cfg.weight_decay, lr_t, b1, b2, 1e-8)[0][0], np.concatenate([p[k] for k in names]), 1e-9)
    # Sterbenz: 1 - float32(0.999) and 1 - float32(0.9) are exact in float32
    for b in (0.9, 0.999):
        assert float(np.float32(1.0) - np.float32(b)) == 1.0 - float(np.float32(b))
    # planted zeros: an element with g = m = v = 0 only decays
    ld, la, b1, b2, eps = X.adamw_hyper()
    (w, m1, v1), _ = X.adamw(p0, g0, m0, v0, ld, la, b1, b2, eps)
    z = (g0 == 0) & (m0 == 0) & (v0 == 0)
    assert int(z.sum()) >= 1 and _same(w[z], p0[z] - ld * p0[z], 1e-16) and float(m1[z].abs().max()) == 0 and float(v1[z].abs().max()) == 0


def test_colsum_and_dense_against_torch():
    for M, N, ld in X.COLSUM_CASES[:6]:
        x, out0 = X.colsum_inputs(M, N, ld)
        v, m = X.colsum(x, out0, M, N, True)
        assert _same(v, out0.double() + torch.from_numpy(np.sum(x.numpy()[:, :N].astype(np.float64), axis=0))) and _covers(m, v)
        assert _same(X.colsum(x, out0, M, N, False)[0], v - out0.double())
    for rows, K, N in X.DENSE_K_CASES:
        x, W, b = X.dense_k_inputs(rows, K, N)
        for gelu_on in (False, True):
            for bias in (b, None):
                a = F.linear(x.double(), W.double().t(), None if bias is None else bias.double())
                v, m = X.dense_small_k(x, W, bias, gelu_on)
                assert _same(v, F.gelu(a) if gelu_on else a) and _covers(m, v)


# ------------------------------------------------------------------ 2. the comparison rejects what these kernels get wrong
def _c(kernel):
    import test_hip_transformer_kernels as G
    return G.C[kernel]


def test_rejects_a_dropped_last_partial_float4_column():
    M, N, ld = 128, 66, 68                                                     # columns 64, 65 are the float4 kernel's tail branch
    x, out0 = X.colsum_inputs(M, N, ld)
    for acc in (False, True):
        want, mag = X.colsum(x, out0, M, N, acc)
        got = want.clone()
        got[64:] = out0.double()[64:] if acc else 0.0
        assert R.rejects(got, want, mag, _c('colsum')) and not R.rejects(X.colsum_f32(x, out0, M, N, ld, acc), want, mag, _c('colsum'))


def test_rejects_a_skipped_last_row_of_a_16_row_block():
    for rows in (16, 37):
        dy, x, gamma, res, dg0, db0 = X.ln_bwd_inputs(rows, 260)
        (dx, dg, db), (mx, mg, mb) = X.layernorm_bwd(dy, x, gamma, X.LN_EPS, res, dg0, db0)
        keep = torch.ones(rows, dtype=torch.bool)
        keep[15] = False                                                       # the fourth row of wave 3 in the first block
        (_, sg, sb), _ = X.layernorm_bwd(dy[keep], x[keep], gamma, X.LN_EPS, None, dg0, db0)
        stale = dx.clone()
        stale[15] = 0.0
        c = _c('layernorm_bwd')
        assert R.rejects(sg, dg, mg, c) and R.rejects(sb, db, mb, c) and R.rejects(stale, dx, mx, c)
        assert not any(R.rejects(g, w, m, c) for g, w, m in zip(X.layernorm_bwd_f32(dy, x, gamma, X.LN_EPS, res, dg0, db0), (dx, dg, db), (mx, mg, mb)))


def test_rejects_a_mask_off_by_one_view():
    for batch, T, L, spec, scale in X.MASK_CASES[:3]:
        s, dp = X.mask_inputs(batch, T, L, spec)
        want, mag = X.softmax_mask(s, T, L, spec, scale)
        for shift in (1, -1):
            assert R.rejects(X.softmax_mask(s, T, L, spec, scale, shift)[0], want, mag, _c('softmax_mask_')), (spec, shift)
        assert not R.rejects(X.softmax_mask_f32(s, T, L, spec, scale), want, mag, _c('softmax_mask_'))
        ds, mds = X.softmax_mask_bwd(want.float(), dp, T, L, spec, scale)
        wrong = X.softmax_mask(s, T, L, spec, scale, 1)[0].float()             # the probabilities of the shifted mask, through the right backward
        assert R.rejects(R.softmax_rows_bwd(wrong, dp, scale)[0], ds, mds, _c('softmax_mask_bwd_'))


def test_rejects_a_missing_uniform_term_of_label_smoothing():
    eps = X.f32(0.1)
    for rows, V in ((5, 65), (1027, 1026), (1, 1)):
        logits, t, w = X.ce_inputs(rows, V)
        w[0] = 0.5                                                             # (a row of weight 0 has no gradient to get wrong)
        (l, dl), (ml, mdl) = X.softmax_ce(logits, t, w, eps)
        bl, bdl = X.softmax_ce_without_uniform_term(logits, t, w, eps)
        assert R.rejects(bl, l, ml, _c('softmax_ce')) and R.rejects(bdl, dl, mdl, _c('softmax_ce'))
        gl, gdl = X.softmax_ce_f32(logits, t, w, eps)
        assert not R.rejects(gl, l, ml, _c('softmax_ce')) and not R.rejects(gdl, dl, mdl, _c('softmax_ce'))


def test_rejects_a_tie_resolved_to_the_higher_index():
    for n, kind in ((65, 'tie_next_lane'), (65, 'tie_same_lane'), (1026, 'tie_same_lane'), (63, 'all_equal'), (64, 'all_neg_inf')):
        x = X.argmax_input(5, n, kind)
        want, _ = X.argmax_rows(x, n)
        assert R.mismatches(X.argmax_rows_last(x, n), want) > 0, (n, kind)
    x = X.argmax_input(5, 64, 'plain')
    assert R.mismatches(X.argmax_rows(x, 64 + X.ARGMAX_PAD)[0], X.argmax_rows(x, 64)[0]) > 0       # a read into the pad


def test_rejects_decay_inside_a_no_decay_range():
    ld, la, b1, b2, eps = X.adamw_hyper()
    p, g, m, v = X.adamw_inputs(X.ADAMW_FLAT_N)
    for name, ranges in X.ADAMW_FLAT_RANGES.items():
        if not ranges:
            continue
        mask = X.nodecay_mask(X.ADAMW_FLAT_N, ranges)
        (w, _, _), (mw, _, _) = X.adamw(p, g, m, v, ld, la, b1, b2, eps, nodecay=mask)
        assert R.rejects(X.adamw(p, g, m, v, ld, la, b1, b2, eps)[0][0], w, mw, _c('adamw_')), name          # decay everywhere
        last = mask.clone()
        last[ranges[-1][1] - 4:ranges[-1][1]] = False                          # the last float4 of the last range decayed
        assert R.rejects(X.adamw(p, g, m, v, ld, la, b1, b2, eps, nodecay=last)[0][0], w, mw, _c('adamw_')), name
        assert not R.rejects(X.adamw_f32(p, g, m, v, ld, la, b1, b2, eps, nodecay=mask)[0], w, mw, _c('adamw_'))
        assert sum(b - a for a, b, nd in X.segments(X.ADAMW_FLAT_N, ranges)) == X.ADAMW_FLAT_N
        assert [(a, b) for a, b, nd in X.segments(X.ADAMW_FLAT_N, ranges) if nd] == ranges


def test_rejects_a_row_offset_by_one_in_the_transpose():
    for rows, cols in X.TRANSPOSE_SHAPES[1:]:
        src = X.transpose_input(rows, cols, 3, 3, False)
        want, _ = X.transpose(src, rows, cols)
        assert R.mismatches(X.transpose(torch.roll(src, 1, 1), rows, cols)[0], want) > 0
        assert R.mismatches(X.transpose(torch.roll(src, 1, 2), rows, cols)[0], want) > 0     # a column off by one: the pad enters


def test_rejects_a_second_lap_that_is_not_run_and_a_wrong_embedding_row():
    u, df = X.gelu_inputs(1028)
    want, mag = X.gelu(u)
    got = want.clone()
    got[-4:] = 0.0
    assert R.rejects(got, want, mag, _c('gelu'))
    BS, L, d, V = X.EMBED_CASES[1]
    ids, wte, wpe, add = X.embed_inputs(BS, L, d, V)
    want, _ = X.embed_sum(ids, wte, wpe, add, BS, L, d)
    assert R.mismatches(X.embed_sum(ids, wte, torch.roll(wpe, 1, 0), add, BS, L, d)[0], want) > 0
    assert R.mismatches(X.embed_sum(ids.clamp(max=V - 2), wte, wpe, add, BS, L, d)[0], want) > 0


# ------------------------------------------------------------------ 3. calibration
def calibration():
    """kernel -> worst |float32 restatement - float64| / (2^-24 x magnitude) over the GPU test's inputs (the second-lap sizes excepted:
    the same formula element by element)"""
    out = {}

    def note(k, *triples):
        out[k] = max([out.get(k, 0.0)] + [R.worst_ratio(g, w, m) for g, w, m in triples])
    for M, N, ld in X.COLSUM_CASES:
        x, out0 = X.colsum_inputs(M, N, ld)
        for acc in (False, True):
            note('colsum', (X.colsum_f32(x, out0, M, N, ld, acc),) + X.colsum(x, out0, M, N, acc))
    eps = X.f32(X.LN_EPS)
    for d in X.LN_D:
        for rows in X.LN_ROWS:
            x, gamma, beta = X.ln_inputs(rows, d)
            note('layernorm', (X.layernorm_f32(x, gamma, beta, eps),) + X.layernorm(x, gamma, beta, eps))
    for rows, d in X.LN_BWD_CASES:
        dy, x, gamma, res, dg0, db0 = X.ln_bwd_inputs(rows, d)
        for acc, with_res in X.LN_BWD_VARIANTS:
            a = (res if with_res else None, dg0 if acc else None, db0 if acc else None)
            want, mag = X.layernorm_bwd(dy, x, gamma, eps, *a)
            note('layernorm_bwd', *zip(X.layernorm_bwd_f32(dy, x, gamma, eps, *a), want, mag))
    for n in X.GELU_SIZES[:2] + [1541]:
        u, df = X.gelu_inputs(n)
        note('gelu', (X.gelu_f32(u),) + X.gelu(u))
        want, mag = X.gelu_bwd(u, df)
        note('gelu_bwd', (X.gelu_bwd_f32(u, df), want, mag))
        note('gelu_bwd bf16', (X.gelu_bwd_fast_f32(u, df).float(), want, X.gelu_bwd_bf16_bound(want, df)))
    for rows, n in X.SOFTMAX_CASES:
        x = X.softmax_logits(rows, n)
        for scale in (1.0, 0.0625):
            note('softmax_rows_', (X.softmax_rows_f32(x, scale),) + X.softmax_rows(x, scale))
    for batch, T, L, spec, scale in X.MASK_CASES:
        s, dp = X.mask_inputs(batch, T, L, spec)
        want, mag = X.softmax_mask(s, T, L, spec, scale)
        note('softmax_mask_', (X.softmax_mask_f32(s, T, L, spec, scale), want, mag))
        p = want.float()
        note('softmax_mask_bwd_', (X.softmax_mask_bwd_f32(p, dp, T, L, spec, scale),) + X.softmax_mask_bwd(p, dp, T, L, spec, scale))
    for rows, V, spread in [(r, v, False) for r in X.CE_ROWS for v in X.CE_V] + [X.CE_SPREAD + (True,)]:
        logits, t, w = X.ce_inputs(rows, V, spread)
        for e in X.CE_SMOOTHING:
            want, mag = X.softmax_ce(logits, t, w, X.f32(e))
            note('softmax_ce', *zip(X.softmax_ce_f32(logits, t, w, X.f32(e)), want, mag))
    hyper = X.adamw_hyper()
    for n in X.ADAMW_SIZES[:2]:
        p, g, m, v = X.adamw_inputs(n)
        want, mag = X.adamw(p, g, m, v, *hyper)
        note('adamw_', *zip(X.adamw_f32(p, g, m, v, *hyper), want, mag))
    p, g, m, v = X.adamw_inputs(X.ADAMW_FLAT_N)
    for ranges in X.ADAMW_FLAT_RANGES.values():
        mask = X.nodecay_mask(X.ADAMW_FLAT_N, ranges)
        want, mag = X.adamw(p, g, m, v, *hyper, nodecay=mask)
        note('adamw_', *zip(X.adamw_f32(p, g, m, v, *hyper, nodecay=mask), want, mag))
    for rows, K, N in X.DENSE_K_CASES:
        x, W, b = X.dense_k_inputs(rows, K, N)
        for gelu_on in (False, True):
            for bias in (b, None):
                note('dense_small_k', (X.dense_small_k_f32(x, W, bias, gelu_on),) + X.dense_small_k(x, W, bias, gelu_on))
    return out


def _pow2_ceil(v):
    return 2.0 ** int(np.ceil(np.log2(max(v, 2.0 ** -20))))


def test_calibration_covers_the_gpu_tests_constants():
    """c = 4 x the float32 CPU restatement's worst error, rounded up to a power of two, and the basis recorded beside it in the GPU test's
    table is this run's.  A restatement's row sums depend on how torch splits them, so the table may sit one binade from this run's
    figure, never further"""
    import test_hip_transformer_kernels as G
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        cal = calibration()
    finally:
        torch.set_num_threads(threads)
    for k in sorted(cal):
        print(f'calibration {k}: fp32 CPU restatement worst {cal[k]:.2f} units of 2^-24 x magnitude -> c = {_pow2_ceil(4 * cal[k]):g} '
              f'(table: c = {G.C[k]:g}, basis {G.BASIS[k]:g})')
    assert set(cal) == set(G.C) == set(G.BASIS)
    for k, v in cal.items():
        assert G.C[k] == _pow2_ceil(4 * G.BASIS[k]), k
        assert _pow2_ceil(4 * v) <= 2 * G.C[k] and G.C[k] <= 2 * _pow2_ceil(4 * v), (k, v, G.C[k])
