"""GPU: the codebook distance table and the code k-NN search (csrc/code_knn.hip, ops.codebook_distances, ops.code_knn) against the
float32 restatements of tests/code_knn_ref.py BIT FOR BIT (the order of operations is fixed: no tolerance, no exemptions), their
footprint (framed.Frame: exactly the logical elements written, no guard touched, nothing beyond row N read), the out-of-range code
rules, and the way up: SceneBank.similar, build_image_match_map, the match map through evaluate_scene, VQGAN.code_distances.

The tile kernel takes TILE = 256 database rows per workgroup and QG = 8 queries per workgroup (CK_TILE, KNN_QG of the sources).
What the restatements themselves are worth is tests/test_code_knn_ref_host.py's business.  Parity facts go through
conftest.parity_report (the measured copy of its ``fact`` lines: profiles/code_knn_parity.txt)."""
import ctypes

import numpy as np
import pytest
import torch

import code_knn_ref as ref
from framed import Frame

pytestmark = pytest.mark.gpu

TILE, QG = 256, 8
NMAX = 2 * TILE + 3
CTX = 4                # context views per query in the evaluator tests (the reference: 19)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib_():
    from viewformer_amd import _lib
    return _lib.load()


def _record(line):
    """one parity fact: a line of conftest.parity_report's file and of stdout"""
    from conftest import parity_report
    parity_report(test='code_knn', fact=line)


# ------------------------------------------------------------------------------------------------ table
@pytest.mark.parametrize('K,D', [(5, 2), (37, 19), (1024, 256)])
def test_table_equals_the_literal_bit_for_bit(dev, K, D):
    from viewformer_amd import _lib, ops
    E, T32, _ = ref.tables(K, D, 3)
    want = torch.from_numpy(np.array(T32))
    Et = torch.from_numpy(np.ascontiguousarray(E.T))                              # feature-major [D][K], as VQGAN._E
    for ld in (K, K + 3):
        src = Frame(D, K, ld, torch.float32, dev).load(Et)
        out = Frame(K, K, K, torch.float32, dev)
        _lib.check(_lib_().vf_codebook_dist_table_f32(_P(src.view), D, K, ld, _P(out.view), _strm()), 'vf_codebook_dist_table_f32')
        torch.cuda.synchronize()
        assert src.violations() == [] and out.violations() == []                  # every element written, no guard touched
        assert torch.equal(out.view.cpu(), want)
    assert torch.equal(ops.codebook_distances(Et.to(dev), D, K).cpu(), want)
    assert torch.equal(ops.codebook_distances(src.view, D, K).cpu(), want)        # a strided codebook
    _record(f'table K={K} D={D}: {K * K} of {K * K} elements bit-equal to table32_literal, ldE in ({K}, {K + 3})')


# ------------------------------------------------------------------------------------------------ search
class _Call:
    """one vf_code_knn_f32 call on framed tensors: db / queries with row gaps (ld = t*t + 5; the gaps hold the int32 sentinel, an
    out-of-range code), idx / dist / workspace framed"""

    def __init__(self, dev, db, q, T32, t):
        self.dev, self.t, self.P = dev, t, t * t
        self.K = T32.shape[0]
        self.table = torch.from_numpy(np.array(T32)).to(dev)
        self.db_np, self.q_np = db, q
        self.frames = {}

    def _input(self, name, a, n):
        key = (name, n)
        if key not in self.frames:
            self.frames[key] = Frame(n, self.P, self.P + 5, torch.int32, self.dev).load(torch.from_numpy(np.array(a[:n])))
        return self.frames[key]

    def run(self, N, qsel, k, window, exclude=None, guard=None):
        """-> (idx int64 [Q,k], dist float32 [Q,k]) of queries ``qsel`` against the first N rows; asserts the footprint"""
        lib = _lib_()
        from viewformer_amd import _lib
        q = self.q_np[qsel]
        Q = len(q)
        fdb = self._input('db', self.db_np, N)
        if ('q', tuple(qsel)) not in self.frames:
            self.frames['q', tuple(qsel)] = Frame(Q, self.P, self.P + 5, torch.int32, self.dev).load(torch.from_numpy(np.array(q)))
        fq = self.frames['q', tuple(qsel)]
        if guard is not None:
            fdb.refill(guard), fq.refill(guard)
        if ('out', Q, k) not in self.frames:
            self.frames['out', Q, k] = Frame(Q, k, k, torch.int32, self.dev), Frame(Q, k, k, torch.float32, self.dev)
        fidx, fdist = self.frames['out', Q, k]
        fidx.ibits.fill_(fidx.sentinel), fdist.ibits.fill_(fdist.sentinel)              # fresh: every byte the sentinel again
        nws = int(lib.vf_code_knn_workspace_bytes(N, Q, k))
        assert nws == (0 if N <= TILE else Q * ((N + TILE - 1) // TILE) * k * 8)
        fws = Frame.raw(max(nws, 8), self.dev)
        ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).to(self.dev)
        _lib.check(lib.vf_code_knn_f32(_P(fdb.view), N, fdb.ld, _P(fq.view), Q, fq.ld, self.t, _P(self.table), self.K, window, _P(ex), k,
                                       _P(fidx.view), _P(fdist.view), _P(fws.view), _strm()), 'vf_code_knn_f32')
        torch.cuda.synchronize()
        assert fdb.violations() == [] and fq.violations() == [], (fdb.violations(), fq.violations())
        assert fidx.violations() == [] and fdist.violations() == [], (fidx.violations(), fdist.violations())
        ws_bad = [v for v in fws.violations() if v[0] != 'unwritten']               # (the workspace's contents are the kernel's own)
        assert ws_bad == [], ws_bad
        if guard is not None:
            fdb.refill(-0x5A5A5A5B), fq.refill(-0x5A5A5A5B)                         # the frames are shared: back to the sentinel
        return fidx.view.cpu().numpy().astype(np.int64), fdist.view.cpu().numpy()


def _inputs(t, K, seed):
    """NMAX database rows and 9 queries: five planted (replaced tokens, shifted), four random"""
    db = ref.code_maps(NMAX, t, K, seed)
    rows = np.array([3, TILE - 2, TILE, NMAX - 1, 7])
    q = np.concatenate((ref.planted_replaced(db, rows[:3], [1, t, t * t // 2], K, seed + 1), ref.planted_shifted(db, rows[3:], t, K, seed + 2),
                        ref.code_maps(4, t, K, seed + 3)))
    return db, q


@pytest.mark.parametrize('t', [3, 8])
@pytest.mark.parametrize('K', [5, 1024])
@pytest.mark.parametrize('wsel', [0, 1, -1])
def test_search_equals_the_literal_bit_for_bit(dev, t, K, wsel):
    """window in {0, 1, t - 1} x k in {1, 5, 32} x Q in {1, 9} x N in {k (k + 1 with exclude), TILE - 1, TILE + 1, 2 TILE + 3} x exclude in
    {absent, all -1, each query's true nearest row}: idx and dist torch.equal to top_rows(distances32_literal)"""
    window = t - 1 if wsel < 0 else wsel
    _, T32, _ = ref.tables(K, 2 if K == 5 else 256, 3)
    db, q = _inputs(t, K, 20 + t)
    d32 = ref.distances32_literal(db, q, T32, t, window)                           # [9,NMAX], once; a prefix of the rows is a prefix of the columns
    call = _Call(dev, db, q, T32, t)
    calls = ties = 0
    for k in (1, 5, 32):
        for qsel in ([4], list(range(9))):
            for mode in ('absent', 'none', 'nearest'):
                for N in (k + (mode != 'absent'), TILE - 1, TILE + 1, NMAX):
                    d = d32[qsel][:, :N]
                    exclude = None if mode == 'absent' else np.full(len(qsel), -1) if mode == 'none' else ref.top_rows(d, 1)[:, 0]
                    want_idx, want_dist = ref.top_rows(d, k, exclude, return_dist=True)
                    idx, dist = call.run(N, qsel, k, window, exclude)
                    assert np.array_equal(idx, want_idx), (k, len(qsel), mode, N)
                    assert np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32)), (k, len(qsel), mode, N)
                    if mode == 'nearest':
                        assert not (idx == exclude[:, None]).any()
                    calls += 1
                    ties += int((np.diff(want_dist, axis=-1) == 0).sum())
    _record(f'search t={t} K={K} window={window}: {calls} of {calls} calls bit-equal in idx and dist (k 1/5/32, Q 1/9, N k..{NMAX}, '
            f'exclude absent/-1/nearest, ld = t*t + 5), {ties} exact ties among the returned neighbours')


def test_search_at_the_largest_grid_and_codebook(dev):
    """t = 16, K = 4096: the shape whose LDS request is the largest (one staged table row per chunk)"""
    t, K = 16, 4096
    g = np.random.default_rng(30)
    T32 = np.abs(g.standard_normal((K, K))).astype(np.float32)                     # (any non-negative table: the search does not ask for symmetry)
    db = ref.code_maps(TILE + 9, t, K, 31)
    q = np.concatenate((ref.planted_replaced(db, [5, TILE + 1], 40, K, 32), ref.code_maps(1, t, K, 33)))
    call = _Call(dev, db, q, T32, t)
    for window in (0, 2):
        want_idx, want_dist = ref.top_rows(ref.distances32_literal(db, q, T32, t, window), 5, return_dist=True)
        idx, dist = call.run(TILE + 9, [0, 1, 2], 5, window)
        assert np.array_equal(idx, want_idx) and np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32))
    _record('search t=16 K=4096 window in (0, 2): 2 of 2 calls bit-equal in idx and dist')


# ------------------------------------------------------------------------------------------------ contract
def test_a_query_alone_and_among_others_and_rows_beyond_n(dev):
    t, K = 8, 1024
    _, T32, _ = ref.tables(K, 256, 3)
    db, q = _inputs(t, K, 40)
    call = _Call(dev, db, q, T32, t)
    for window, N in ((0, NMAX), (1, TILE + 1), (1, 40)):
        idx, dist = call.run(N, list(range(9)), 19, window)
        for i in range(9):                                                         # Q = 1 against Q = 9: one more than a query group
            i1, d1 = call.run(N, [i], 19, window)
            assert np.array_equal(i1[0], idx[i]) and np.array_equal(d1[0].view(np.uint32), dist[i].view(np.uint32))
        # nothing outside the logical windows is read: valid codes in every guard and row gap (the default sentinel is an out-of-range
        # code, which the selection would never show), results unchanged; with N = k every row is returned, so a row read beyond N
        # would have to displace one
        for guard in (0, K - 1):
            i2, d2 = call.run(N, list(range(9)), 19, window, guard=guard)
            assert np.array_equal(i2, idx) and np.array_equal(d2.view(np.uint32), dist.view(np.uint32))
    idx, _ = call.run(19, list(range(9)), 19, 1, guard=0)
    assert (np.sort(idx, -1) == np.arange(19)).all()
    # ops.code_knn is that call: [N,t,t] and [N,t*t], strided rows, with and without distances
    from viewformer_amd import ops
    want_idx, want_dist = call.run(NMAX, list(range(9)), 19, 1)
    dbt, qt = torch.from_numpy(db).to(dev), torch.from_numpy(q).to(dev)
    for a, b in ((dbt, qt), (dbt.view(-1, t, t), qt.view(-1, t, t)), (call._input('db', db, NMAX).view, qt)):
        idx, dist = ops.code_knn(a, b, call.table, 19, window=1, return_dist=True)
        assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and tuple(idx.shape) == tuple(dist.shape) == (9, 19)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(dist.cpu().numpy().view(np.uint32), want_dist.view(np.uint32))
        assert torch.equal(ops.code_knn(a, b, call.table, 19, window=1), idx)
    ex = want_idx[:, 0]
    assert np.array_equal(ops.code_knn(dbt, qt, call.table, 18, window=1, exclude=ex.tolist()).cpu().numpy(), want_idx[:, 1:])
    assert np.array_equal(ops.code_knn(dbt, qt, call.table, 18, window=1, exclude=torch.from_numpy(ex).to(dev)).cpu().numpy(), want_idx[:, 1:])
    for bad in (dict(k=0), dict(k=33), dict(k=NMAX + 1), dict(k=5, window=t), dict(k=5, window=-1), dict(k=NMAX, exclude=ex.tolist()),
                dict(k=5, exclude=[1, 2])):
        with pytest.raises(ValueError):
            ops.code_knn(dbt, qt, call.table, **bad)
    _record('contract: Q = 1 == Q = 9 row by row (27 queries), valid codes in guards and row gaps change nothing (6 calls), ops.code_knn == the raw call')


def test_out_of_range_codes_and_nan_entries_follow_the_rules(dev):
    """codes of -1, K and 2^31 - 1 in database rows and in queries, NaN table entries: what the host restatement says, bit for bit"""
    t = 3
    for K in (5, 1024):
        _, T32, _ = ref.tables(K, 2 if K == 5 else 256, 3)
        db, q = (np.array(x) for x in _inputs(t, K, 50))
        db[4, :] = [-1, K, 2 ** 31 - 1] * 3                                        # a row without a single valid candidate: +inf, last
        db[5, 4] = K
        db[TILE + 2, [0, 8]] = [-1, 2 ** 31 - 1]
        db[9::50, 2] = -(2 ** 31)
        q[1, 8] = -1                                                               # a query with an invalid token: every distance +inf
        q[6, 0] = K
        q[7, 3] = 2 ** 31 - 1
        Tn = np.array(T32)
        if K != 5:                                                                 # (on the lattice every query holds every code)
            Tn[q[0, 0], :] = np.nan                                                # every candidate of query 0's first token: that term is +inf
        Tn[q[2, 4], db[::3, 0] if K != 5 else db[:1, 0]] = np.nan                  # some candidates of query 2's centre token: they never enter
        call = _Call(dev, db, q, Tn, t)
        for window in (0, 1, 2):
            d = ref.distances32_literal(db, q, Tn, t, window)
            assert not np.isnan(d).any() and np.isinf(d[[1, 6, 7] + [0] * (K != 5)]).all() and np.isinf(d[:, 4]).all()
            # row 5's hole is the ONLY candidate of the centre token at window 0: +inf there, finite once the window holds others
            assert np.isinf(d[2, 5]) if window == 0 else np.isfinite(d[2, 5])
            assert 0.3 < np.isfinite(d).mean() < 0.8
            for N, k in ((NMAX, 32), (TILE - 1, 5), (6, 6)):
                want_idx, want_dist = ref.top_rows(d[:, :N], k, return_dist=True)
                idx, dist = call.run(N, list(range(9)), k, window)
                assert np.array_equal(idx, want_idx) and np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32)), (K, window, N)
            assert list(call.run(NMAX, [1], 5, window)[0][0]) == [0, 1, 2, 3, 4]    # all +inf: a tie, the lowest indices
    _record('out-of-range codes (-1, K, 2^31 - 1, -2^31) and NaN table entries: 18 of 18 calls bit-equal to the restatement')


# ------------------------------------------------------------------------------------------------ through the bank and the evaluator
@pytest.fixture(scope='module')
def world(dev):
    from viewformer_amd.config import MIGTConfig, VQGANConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.scene_bank import SceneBank
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, make_vqgan_weights, synthetic_scene_batch
    vcfg = VQGANConfig(ch=32, ch_mult=[1, 2, 4], num_res_blocks=1, attn_resolutions=[16], image_size=32, z_channels=32, embed_dim=32,
                       n_embed=128)
    mcfg = MIGTConfig(n_embeddings=128, n_head=2, d_model=128, n_layer=2, token_image_size=8, sequence_size=CTX + 1, pose_multiplier=0.2,
                      localization_weight='1')
    vsd = make_vqgan_weights(vcfg, seed=1, codebook_scale=0.05)
    msd = make_migt_weights(mcfg, seed=1, std=0.05)
    vq_m = VQGAN(vcfg, data_format='NHWC').load_state_dict(vsd).to(dev)
    tr_m = MIGT(mcfg).load_state_dict(msd).to(dev)
    frames, cams = synthetic_scene_batch(1, 40, 32, seed=21)
    bank = SceneBank(vq_m, torch.from_numpy(frames[0]), cams[0], batch_size=16)          # chunks of 16, 16 and 8 frames
    qf, qc = synthetic_scene_batch(6, 1, 32, seed=22)
    queries = [(torch.from_numpy(qf[b]), qc[b], f'seq-03/frame-{b:06d}') for b in range(6)]
    queries[2] = (torch.from_numpy(frames[0][11:12]), qc[2], queries[2][2])              # one query IS a bank frame
    return dict(vcfg=vcfg, vsd=vsd, vq=vq_m, tr=tr_m, bank=bank, frames=torch.from_numpy(frames[0]), queries=queries)


def test_bank_similar(dev, world):
    from viewformer_amd import ops
    bank, vq_m = world['bank'], world['vq']
    assert bank.codebook_model is vq_m and tuple(bank.codes.shape) == (40, 8, 8)
    codes = bank.codes.cpu().numpy().reshape(40, -1)
    assert len({row.tobytes() for row in codes}) == 40                             # (no two frames share a code map: "itself" is well defined)
    for i in (0, 16, 39):
        assert int(bank.similar(images=bank.frames[i:i + 1], k=1)[0, 0]) == i
        idx, dist = bank.similar(images=bank.frames[i:i + 1], k=3, exclude=[i], return_dist=True)
        assert i not in idx[0].tolist() and float(dist[0, 0]) > 0
        assert float(bank.similar(codes=bank.codes[i:i + 1], k=1, return_dist=True)[1][0, 0]) == 0.0
    sel = torch.tensor([3, 17, 38])
    for window in (0, 2):
        a = bank.similar(images=bank.frames[sel], k=5, window=window, return_dist=True)
        b = bank.similar(codes=bank.codes[sel.to(dev)], k=5, window=window, return_dist=True)
        c = ops.code_knn(bank.codes, bank.codes[sel.to(dev)], vq_m.code_distances(), 5, window, return_dist=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        assert a[0][:, 0].tolist() == sel.tolist()
    # int64 codes on the host are taken too; exactly one of codes / images
    assert torch.equal(bank.similar(codes=bank.codes[sel.to(dev)].cpu().long(), k=5, window=2), a[0])
    for kw in (dict(), dict(codes=bank.codes[:1], images=bank.frames[:1]), dict(codes=bank.codes[:1, :4, :4]), dict(images=bank.frames[:1].float())):
        with pytest.raises(ValueError):
            bank.similar(k=1, **kw)
    # the restatement on the model's own codebook: the table, and the search on the bank's codes
    E = vq_m._E.cpu().numpy().T                                                    # [K,D]
    T32 = ref.table32_literal(E)
    assert torch.equal(vq_m.code_distances().cpu(), torch.from_numpy(T32))
    want_idx, want_dist = ref.top_rows(ref.distances32_literal(codes, codes[sel.numpy()], T32, 8, 2), 5, return_dist=True)
    assert np.array_equal(a[0].cpu().numpy(), want_idx) and np.array_equal(a[1].cpu().numpy().view(np.uint32), want_dist.view(np.uint32))


def test_code_distances_are_cached_and_follow_the_weights(dev, world):
    from viewformer_amd import ops
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_vqgan_weights
    vcfg = world['vcfg']
    vq2 = VQGAN(vcfg, data_format='NHWC').load_state_dict(world['vsd']).to(dev)
    a = vq2.code_distances()
    assert vq2.code_distances() is a and tuple(a.shape) == (128, 128) and torch.equal(a, world['vq'].code_distances())
    vq2.load_state_dict(make_vqgan_weights(vcfg, seed=2, codebook_scale=0.05))
    b = vq2.code_distances()
    assert b is not a and vq2.code_distances() is b and not torch.equal(a, b)
    assert torch.equal(b, ops.codebook_distances(vq2._E, vcfg.embed_dim, vcfg.n_embed))


def test_match_map_from_the_bank_through_the_evaluator(dev, world, tmp_path):
    from viewformer_amd import ops
    from viewformer_amd.evaluate_sevenscenes import build_image_match_map, evaluate_scene, load_image_match_map, save_image_match_map
    bank, vq_m, tr_m, queries = world['bank'], world['vq'], world['tr'], world['queries']
    mm = build_image_match_map(bank, queries, top_n=3, window=1, batch_size=4)       # batches of 4 and 2
    assert list(mm) == [f + '.color.png' for _, _, f in queries] and all(len(v) == 3 for v in mm.values())
    qcodes = vq_m.encode(torch.cat([f for f, _, _ in queries]).to(dev))[-1].to(torch.int32)
    idx = ops.code_knn(bank.codes, qcodes, vq_m.code_distances(), 3, window=1).cpu().tolist()
    by_hand = {f + '.color.png': [bank.files[i] for i in row] for (_, _, f), row in zip(queries, idx)}
    assert mm == by_hand and type(by_hand) is dict
    assert mm[queries[2][2] + '.color.png'][0] == bank.files[11]                     # the query that is a bank frame finds it first
    assert build_image_match_map(bank, queries, top_n=3, window=1, batch_size=1) == mm
    kw = dict(generation_procedure='standard', batch_size=2, top_n_matched_images=2, context_size=CTX, seed=5)
    got = evaluate_scene(bank, tr_m, vq_m, queries, match_map=mm, **kw)
    want = evaluate_scene(bank, tr_m, vq_m, queries, match_map=by_hand, **kw)
    assert list(got) == list(want) and all(np.isfinite(v) for v in want.values()) and all(got[k] == want[k] for k in want), (got, want)
    p = tmp_path / 'matches.txt'
    save_image_match_map(str(p), mm)
    loaded = load_image_match_map(str(p))
    assert loaded == mm
    again = evaluate_scene(bank, tr_m, vq_m, queries, match_map=loaded, **kw)
    assert all(again[k] == want[k] for k in want)
    # the matches do reach the context: without a map the random fill gives another result
    plain = evaluate_scene(bank, tr_m, vq_m, queries, **dict(kw, top_n_matched_images=0))
    assert any(plain[k] != want[k] for k in want)
