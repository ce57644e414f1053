"""CPU: the restatements the code k-NN kernel is judged by (tests/code_knn_ref.py) against independent fp64 formulations, the cases
the GPU test relies on, the C-ABI of csrc/code_knn.hip without a GPU (argument validation happens before any launch; pointers are never
dereferenced), and the match-map file round trip.

Rank agreement of the float32 literal with fp64 (tol = 4 x the largest |literal - fp64| over every query's fp64 top-(k + 1); a query is
exempt when two of its first k + 1 fp64 distances are within 2 tol).  Measured, cases in the order of RANK_CASES:
    t=8 K=1024 D=256 N=1000 Q=32 k=19 w=0: tol 4.9e-02, exempt 0.031, index lists equal 31/32
    t=8 K=1024 D=256 N=1000 Q=32 k=19 w=1: tol 4.1e-02, exempt 0.000, index lists equal 32/32
    t=8 K=1024 D=256 N=1000 Q=32 k=5  w=7: tol 3.2e-02, exempt 0.000, index lists equal 32/32
    t=3 K=37   D=19  N=300  Q=32 k=5  w=1: tol 9.4e-05, exempt 0.031, index lists equal 32/32
(distances are of the order of t*t * 2 D = 3e4 at D = 256, where a float32 ulp is 2e-3: the tolerances are a few ulps of the sums)."""
import ctypes

import numpy as np
import pytest
import torch

import code_knn_ref as ref

RANK_CASES = [(8, 1024, 256, 1000, 19, 0), (8, 1024, 256, 1000, 19, 1), (8, 1024, 256, 1000, 5, 7), (3, 37, 19, 300, 5, 1)]


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize('K,D', [(5, 2), (37, 19), (1024, 256)])
def test_table_literal_symmetric_zero_diagonal_and_within_the_first_order_bound(K, D):
    E, T32, T64 = ref.tables(K, D, 3)
    assert T32.dtype == np.float32 and T32.shape == (K, K)
    assert np.array_equal(T32, T32.T) and (np.diag(T32) == 0).all() and (T32 >= 0).all()
    # all terms are non-negative: 3 roundings per term and D - 1 additions, to first order (D + 2) 2^-24 relative
    err = np.abs(T32.astype(np.float64) - T64)
    print(f'K={K} D={D}: largest error / bound {float((err / np.maximum((D + 2) * 2.0 ** -24 * T64, 1e-300)).max()):.3f}')
    assert (err <= (D + 2) * 2.0 ** -24 * T64).all()
    if (K, D) == (5, 2):
        assert np.array_equal(T32, np.array([[0, 1, 1, 1, 1], [1, 0, 2, 4, 2], [1, 2, 0, 2, 4], [1, 4, 2, 0, 2], [1, 2, 4, 2, 0]], dtype=np.float32))


# ------------------------------------------------------------------------------------------------ distances
def test_window_zero_is_the_squared_distance_of_the_quantised_latent_maps():
    t, K, D = 4, 37, 19
    E, T32, T64 = ref.tables(K, D, 3)
    db, q = ref.code_maps(50, t, K, 1), ref.code_maps(7, t, K, 2)
    E64 = E.astype(np.float64)
    zq, zm = E64[q], E64[db]                                                       # embed_code: [Q,P,D], [N,P,D]
    want = ((zq[:, None] - zm[None]) ** 2).sum((-1, -2))
    got = ref.distances64(db, q, T64, t, 0)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    lit = ref.distances32_literal(db, q, T32, t, 0)
    assert lit.dtype == np.float32 and np.abs(lit - want).max() <= (D + 2 + t * t) * 2.0 ** -24 * want.max()
    # [n,t,t] maps are read row-major
    assert np.array_equal(ref.distances32_literal(db.reshape(-1, t, t), q.reshape(-1, t, t), T32, t, 0), lit)


def test_full_window_is_the_brute_force_chamfer_distance():
    t, K, D = 3, 37, 19
    _, T32, T64 = ref.tables(K, D, 3)
    db, q = ref.code_maps(20, t, K, 4), ref.code_maps(5, t, K, 5)
    want = ref.chamfer_brute(db, q, T64, t)
    assert np.abs(ref.distances64(db, q, T64, t, t - 1) - want).max() <= 1e-12 * want.max()
    assert np.abs(ref.distances32_literal(db, q, T32, t, t - 1) - want).max() <= 1e-5 * want.max()
    # windows grow monotonically: a larger window can only lower a distance
    d = [ref.distances64(db, q, T64, t, w) for w in range(t)]
    assert all((d[w + 1] <= d[w]).all() for w in range(t - 1)) and (d[1] < d[0]).any()


def test_planted_neighbours_are_found():
    t, K, D, N = 8, 1024, 256, 300
    _, T32, T64 = ref.tables(K, D, 3)
    db = ref.code_maps(N, t, K, 6)
    rows = np.arange(0, N, 9)
    r = 1 + np.arange(len(rows)) % 32                                             # 1 .. 32 = t*t / 2 tokens replaced
    qa = ref.planted_replaced(db, rows, r, K, 7)
    assert ((qa != db[rows]).sum(-1) <= r).all() and ((qa != db[rows]).sum(-1) >= r - 2).all()
    for w in (0, 1, t - 1):
        assert np.array_equal(ref.top_rows(ref.distances64(db, qa, T64, t, w), 1)[:, 0], rows), w
        assert np.array_equal(ref.top_rows(ref.distances32_literal(db, qa, T32, t, w), 1)[:, 0], rows), w
    qb = ref.planted_shifted(db, rows, t, K, 8)
    assert np.array_equal(qb.reshape(-1, t, t)[:, :, 1:], db[rows].reshape(-1, t, t)[:, :, :-1])
    assert np.array_equal(ref.top_rows(ref.distances64(db, qb, T64, t, 1), 1)[:, 0], rows)
    assert np.array_equal(ref.top_rows(ref.distances32_literal(db, qb, T32, t, 1), 1)[:, 0], rows)
    # at w = 1 seven of a shifted query's eight columns find their partner at distance 0: only the vacated column costs anything
    d1 = ref.distances64(db, qb, T64, t, 1)[np.arange(len(rows)), rows]
    d0 = ref.distances64(db, qb, T64, t, 0)[np.arange(len(rows)), rows]
    assert (d1 < 0.25 * d0).all()


@pytest.mark.parametrize('t,K,D,N,k,w', RANK_CASES)
def test_literal_ranks_as_fp64_does(t, K, D, N, k, w):
    """figures in the module docstring"""
    _, T32, T64 = ref.tables(K, D, 3)
    db = ref.code_maps(N, t, K, 10 + t)
    rows = (np.arange(32) * 29) % N
    q = ref.planted_replaced(db, rows, 1 + np.arange(32) % min(32, t * t - 1), K, 11)
    d32, d64 = ref.distances32_literal(db, q, T32, t, w), ref.distances64(db, q, T64, t, w)
    tol, exempt, agree = ref.rank_agreement(d32, d64, k)
    print(f't={t} K={K} D={D} N={N} Q=32 k={k} w={w}: tol {tol:.1e}, exempt {exempt.mean():.3f}, index lists equal {int(agree.sum())}/32')
    assert exempt.mean() <= 0.05
    assert agree[~exempt].all()
    # leave-one-out: with the planted row excluded it is gone and the rest moves up
    tol, exempt, agree = ref.rank_agreement(d32, d64, k, exclude=rows)
    assert exempt.mean() <= 0.05 and agree[~exempt].all()
    top = ref.top_rows(d32, k, exclude=rows)
    assert not (top == rows[:, None]).any()
    plain = ref.top_rows(d32, k)
    first = plain[:, 0] == rows                                                   # (where the planted row was first)
    assert first.mean() > 0.5 and np.array_equal(top[first, :k - 1], plain[first, 1:])


# ------------------------------------------------------------------------------------------------ mutants
def _mutant(db, q, T32, t, w, descending=False, seed_first=False, unclipped=False):
    """distances32_literal with one rule broken"""
    db, q = np.asarray(db, dtype=np.int64), np.asarray(q, dtype=np.int64)
    P = t * t
    acc = None
    for p in (range(P - 1, -1, -1) if descending else range(P)):
        py, px = divmod(p, t)
        if unclipped:                                                             # the window in flat indices: it wraps round the rows' ends
            win = [pp for dy in range(-w, w + 1) for dx in range(-w, w + 1) for pp in [(py + dy) * t + px + dx] if 0 <= pp < P]
        else:
            win = ref._windows(t, w)[p]
        rows = T32[q[:, p]]
        m = rows[:, db[:, win[0]]] if seed_first else np.full((len(q), len(db)), ref.INF32, dtype=np.float32)
        for pp in win:
            cand = rows[:, db[:, pp]]
            m = np.where(cand < m, cand, m)
        acc = m if acc is None else acc + m
    return acc


def test_the_shared_cases_reject_four_mutants():
    t, K, D = 8, 1024, 256
    _, T32, _ = ref.tables(K, D, 3)
    db, q = ref.code_maps(40, t, K, 12), np.array(ref.code_maps(9, t, K, 13))
    q[0, 0] = min(set(range(K)) - set(q[1:].ravel().tolist()))                    # a code no other query holds
    lit = ref.distances32_literal(db, q, T32, t, 1)
    assert np.array_equal(_mutant(db, q, T32, t, 1), lit)                         # the unbroken restatement of the restatement
    # a descending-p sum: other bits
    assert (_mutant(db, q, T32, t, 1, descending=True) != lit).mean() > 0.1
    # the window not clipped at the border
    assert (_mutant(db, q, T32, t, 1, unclipped=True) != lit).mean() > 0.1
    # the minimum seeded with the first candidate: a NaN table entry leaks; by the rule it never enters
    Tn = np.array(T32)
    Tn[q[0, 0], :] = np.nan                                                       # every candidate of query 0's first token
    Tn[q[1, 9], db[:, 0]] = np.nan                                                # the first candidate of query 1's token (1, 1)
    lit_n = ref.distances32_literal(db, q, Tn, t, 1)
    assert not np.isnan(lit_n).any() and np.isinf(lit_n[0]).all() and np.isfinite(lit_n[1:]).all()
    assert np.isnan(_mutant(db, q, Tn, t, 1, seed_first=True)[:2]).all()
    # ties to the highest index: on the lattice nearly every distance is a tie
    _, L32, _ = ref.tables(5, 2, 0)
    dbl, ql = ref.code_maps(60, 3, 5, 14), ref.code_maps(9, 3, 5, 15)
    d = ref.distances32_literal(dbl, ql, L32, 3, 1)
    assert all(len(np.unique(row)) < 30 for row in d)
    low = ref.top_rows(d, 5)
    high = np.stack([np.lexsort((-np.arange(d.shape[1]), row))[:5] for row in d])
    assert (low != high).any(-1).all()
    assert np.array_equal(np.take_along_axis(d, low, -1), np.take_along_axis(d, high, -1))
    for row, got in zip(d, low):                                                  # the lowest index of every tie, by hand
        order = sorted(range(len(row)), key=lambda i: (row[i], i))
        assert list(got) == order[:5]


def test_out_of_range_codes_in_the_restatement():
    t, K = 3, 5
    _, L32, _ = ref.tables(5, 2, 0)
    db, q = ref.code_maps(12, t, K, 16), ref.code_maps(3, t, K, 17)
    clean = ref.distances32_literal(db, q, L32, t, 1)
    bad_db = np.array(db)
    bad_db[4, :] = [-1, K, 2 ** 31 - 1] * 3                                       # a row without a single valid candidate
    bad_db[5, 4] = K                                                              # one hole in the middle
    d = ref.distances32_literal(bad_db, q, L32, t, 1)
    assert np.isinf(d[:, 4]).all() and np.isfinite(d[:, 5]).all() and (d[:, 5] >= clean[:, 5]).all()
    keep = [i for i in range(12) if i not in (4, 5)]
    assert np.array_equal(d[:, keep], clean[:, keep])
    bad_q = np.array(q)
    bad_q[1, 8] = -1
    d = ref.distances32_literal(db, bad_q, L32, t, 1)
    assert np.isinf(d[1]).all() and np.array_equal(d[[0, 2]], clean[[0, 2]])
    assert list(ref.top_rows(d, 3)[1]) == [0, 1, 2]                               # all +inf: a tie, the lowest indices


# ------------------------------------------------------------------------------------------------ C-ABI without a GPU
@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_are_exported_and_the_abi_number_stays(lib):
    from viewformer_amd import _lib
    for name in ('vf_codebook_dist_table_f32', 'vf_code_knn_workspace_bytes', 'vf_code_knn_f32'):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.vf_abi_version() == 20                                             # the additions are additive


def test_table_abi_validation_without_gpu(lib):
    d = ctypes.c_void_p(4096)                                                     # never dereferenced
    tab = lib.vf_codebook_dist_table_f32
    assert tab(None, 256, 1024, 1024, d, None) == -1                              # NULL E
    assert tab(d, 256, 1024, 1024, None, None) == -1                              # NULL table
    assert tab(ctypes.c_void_p(4098), 256, 1024, 1024, d, None) == -1             # misaligned E
    assert tab(d, 256, 1024, 1024, ctypes.c_void_p(4097), None) == -1             # misaligned table
    assert tab(d, 256, 1024, 1023, d, None) == -1                                 # ldE < K
    assert tab(d, 256, 0, 1024, d, None) == -2                                    # K = 0
    assert tab(d, 256, 4097, 4097, d, None) == -2                                 # K > 4096
    assert tab(d, 0, 1024, 1024, d, None) == -2                                   # D = 0


def test_code_knn_abi_validation_without_gpu(lib):
    d = ctypes.c_void_p(4096)                                                     # never dereferenced
    raw, ws = lib.vf_code_knn_f32, lib.vf_code_knn_workspace_bytes

    def knn(db=d, N=7000, ld_db=64, queries=d, Q=4, ld_q=64, t=8, table=d, K=1024, window=0, exclude=None, k=19, idx=d, dist=d,
            workspace=d):
        return raw(db, N, ld_db, queries, Q, ld_q, t, table, K, window, exclude, k, idx, dist, workspace, None)

    assert knn(k=0) == -1 and knn(k=33) == -2                                     # k in [1, 32]
    assert knn(N=18) == -1                                                        # N < k
    assert knn(N=19, exclude=d) == -1                                             # leave-one-out needs k <= N - 1
    assert knn(Q=-1) == -1
    assert knn(N=1 << 31) == -2                                                   # N > 2^31 - 1
    assert knn(t=0) == -1 and knn(t=17, ld_db=289, ld_q=289) == -2                # t in [1, 16]
    assert knn(window=-1) == -1 and knn(window=8) == -1                           # window in [0, t - 1]
    assert knn(K=0) == -1 and knn(K=4097) == -2                                   # K in [1, 4096]
    assert knn(ld_db=63) == -1 and knn(ld_q=63) == -1                             # rows shorter than a code map
    assert knn(db=None) == -1 and knn(queries=None) == -1 and knn(table=None) == -1 and knn(idx=None) == -1
    assert knn(workspace=None) == -1                                              # NULL workspace where one is needed
    assert knn(workspace=ctypes.c_void_p(4100)) == -1                             # workspace alignment
    for name in ('db', 'queries', 'table', 'exclude', 'idx', 'dist'):
        assert knn(**{name: ctypes.c_void_p(4098)}) == -1, name                   # 4-byte alignment
    assert knn(Q=(65535 * 8) + 1) == -2                                           # more query groups than a grid dimension holds
    assert knn(Q=0) == 0 and knn(Q=0, db=None, queries=None, table=None, idx=None, dist=None, workspace=None) == 0     # a no-op
    # workspace: [Q][tiles of 256 rows][k] 8-byte keys; none for a single tile; monotone in N; 0 for invalid shapes
    assert ws(7000, 64, 19) == 64 * 28 * 19 * 8 and ws(256, 64, 9) == 0 and ws(257, 1, 1) == 2 * 8
    sizes = [ws(n, 16, 19) for n in (19, 255, 256, 257, 7000, 100000, (1 << 31) - 1)]
    assert sizes == sorted(sizes) and sizes[-1] == 16 * (1 << 23) * 19 * 8
    assert ws(7000, 4, 0) == 0 and ws(7000, 4, 33) == 0 and ws(8, 4, 9) == 0 and ws(7000, -1, 9) == 0 and ws(1 << 31, 4, 9) == 0
    assert ws(7000, 0, 9) == 0


def test_ops_refuse_before_any_launch(lib):
    from viewformer_amd import ops
    codes, table = torch.zeros((10, 8, 8), dtype=torch.int32), torch.zeros((16, 16))
    for args in ((codes, codes[:2], table, 3),                                    # CPU tensors
                 (codes.long(), codes[:2], table, 3), (codes, codes[:2].float(), table, 3),      # not int32
                 (codes, torch.zeros((2, 4, 4), dtype=torch.int32), table, 3),    # another grid
                 (torch.zeros((10, 8, 7), dtype=torch.int32), codes[:2], table, 3),
                 (torch.zeros((10, 60), dtype=torch.int32), torch.zeros((2, 60), dtype=torch.int32), table, 3)):
        with pytest.raises(ValueError):
            ops.code_knn(*args)
    with pytest.raises(ValueError):
        ops.codebook_distances(torch.zeros((4, 16)), 4, 16)                       # a CPU codebook
    with pytest.raises(ValueError):
        ops.codebook_distances(torch.zeros((4, 16), dtype=torch.float64), 4, 16)


# ------------------------------------------------------------------------------------------------ match map files
def test_match_map_round_trip(tmp_path):
    from viewformer_amd.evaluate_sevenscenes import load_image_match_map, save_image_match_map
    mm = {'seq-03/frame-000001.color.png': ['seq-01/frame-000030.color.png', 'seq-01/frame-000003.color.png', 'seq-02/frame-000017.color.png'],
          'seq-03/frame-000002.color.png': ['seq-01/frame-000009.color.png']}
    p = tmp_path / 'matches.txt'
    save_image_match_map(str(p), mm)
    assert p.read_text().splitlines()[:2] == ['seq-03/frame-000001.color.png seq-01/frame-000030.color.png',
                                              'seq-03/frame-000001.color.png seq-01/frame-000003.color.png']
    back = load_image_match_map(str(p))
    assert back == mm and dict(back) == mm and list(back) == list(mm)
    assert back.get('seq-03/frame-000001.color.png', [])[:2] == mm['seq-03/frame-000001.color.png'][:2]
    with pytest.raises(ValueError):
        save_image_match_map(str(p), {'a b.color.png': ['c']})
