"""Restatements of the code k-NN search (csrc/code_knn.hip, ops.code_knn) on numpy, shared by the host and the GPU tests:

    T[a][b]  = ||e_a - e_b||^2
    d_w(q,m) = sum_p  min_{p' in W_w(p)}  T[q[p]][m[p']]          (W_w(p): Chebyshev distance <= w on the t x t grid, clipped at the border)

in fp64 (``table64``, ``distances64``: the yardstick) and in float32 in the kernel's own operation order (``table32_literal``,
``distances32_literal``: what the kernel must reproduce bit for bit), the selection (``top_rows``: a stable order on (distance bits,
index), NaN canonical and last), and the makers of the inputs the tests share."""
import functools

import numpy as np

INF32 = np.float32(np.inf)


# ------------------------------------------------------------------------------------------------ tables
def table64(E):
    """E [K,D] (one embedding per row) -> fp64 [K,K]"""
    E = np.asarray(E, dtype=np.float64)
    T = np.zeros((E.shape[0], E.shape[0]), dtype=np.float64)
    for j in range(E.shape[1]):                                          # (a loop over j on [K,K] arrays: no [K,K,D] temporary)
        d = E[:, None, j] - E[None, :, j]
        T += d * d
    return T


def table32_literal(E):
    """float32, the kernel's order: T = (((0 + fl(fl(a_0 - b_0)^2)) + fl(fl(a_1 - b_1)^2)) + ...), every operation rounded to float32"""
    E = np.asarray(E, dtype=np.float32)
    K, D = E.shape
    T = np.zeros((K, K), dtype=np.float32)
    for j in range(D):
        d = E[:, None, j] - E[None, :, j]
        T = T + d * d
    assert T.dtype == np.float32
    return T


# ------------------------------------------------------------------------------------------------ distances
def _windows(t, w):
    """for each grid position p (row-major) the positions of W_w(p), clipped at the border"""
    out = []
    for py in range(t):
        for px in range(t):
            out.append([y * t + x for y in range(max(py - w, 0), min(py + w, t - 1) + 1) for x in range(max(px - w, 0), min(px + w, t - 1) + 1)])
    return out


def distances64(db, q, T64, t, w):
    """db [N,t*t], q [Q,t*t] with codes in [0, K) -> fp64 [Q,N]"""
    db, q = np.asarray(db).reshape(len(db), -1)[:, :t * t], np.asarray(q).reshape(len(q), -1)[:, :t * t]
    out = np.zeros((q.shape[0], db.shape[0]), dtype=np.float64)
    for p, win in enumerate(_windows(t, w)):
        rows = T64[q[:, p]]                                              # [Q,K]
        cand = np.stack([rows[:, db[:, pp]] for pp in win], 0)           # [|W|,Q,N]
        out += cand.min(0)
    return out


def distances32_literal(db, q, T32, t, w):
    """float32 [Q,N] in the kernel's order: per position the minimum starts at +inf and takes a candidate iff candidate < current (NaN
    never enters); the sum runs over p ascending, starting from the first term; a query code outside [0, K) makes its term +inf, a
    database code outside [0, K) is skipped as a candidate.  Only the first t*t entries of a row are read."""
    db, q = np.asarray(db).reshape(len(db), -1)[:, :t * t].astype(np.int64), np.asarray(q).reshape(len(q), -1)[:, :t * t].astype(np.int64)
    T32 = np.asarray(T32, dtype=np.float32)
    K = T32.shape[0]
    db_ok = (db >= 0) & (db < K)
    db_c = np.where(db_ok, db, 0)
    acc = None
    for p, win in enumerate(_windows(t, w)):
        q_ok = (q[:, p] >= 0) & (q[:, p] < K)
        rows = T32[np.where(q_ok, q[:, p], 0)]                           # [Q,K]
        m = np.full((q.shape[0], db.shape[0]), INF32, dtype=np.float32)
        for pp in win:
            cand = rows[:, db_c[:, pp]]                                  # [Q,N]
            take = (cand < m) & db_ok[None, :, pp]
            m = np.where(take, cand, m)
        m = np.where(q_ok[:, None], m, INF32).astype(np.float32)
        acc = m if acc is None else acc + m
        assert acc.dtype == np.float32
    return acc


def chamfer_brute(db, q, T64, t):
    """the full one-sided Chamfer distance, position by position: sum_p min over ALL p' (fp64 [Q,N])"""
    out = np.zeros((len(q), len(db)))
    for i, qq in enumerate(np.asarray(q).reshape(len(q), -1)):
        for j, m in enumerate(np.asarray(db).reshape(len(db), -1)):
            out[i, j] = sum(min(T64[a][b] for b in m) for a in qq)
    return out


# ------------------------------------------------------------------------------------------------ selection
def keys(d, exclude=None):
    """uint64 [Q,N]: (distance bits << 32) | index, NaN canonical (0x7FC00000), the excluded row of each query ~0"""
    d = np.ascontiguousarray(d, dtype=np.float32)
    bits = d.view(np.uint32).astype(np.uint64)
    bits = np.where(np.isnan(d), np.uint64(0x7FC00000), bits)
    k = (bits << np.uint64(32)) | np.arange(d.shape[1], dtype=np.uint64)[None, :]
    if exclude is not None:
        ex = np.asarray(exclude).reshape(-1)
        for i, e in enumerate(ex):
            if 0 <= e < d.shape[1]:
                k[i, e] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


def top_rows(d, k, exclude=None, return_dist=False):
    """the k smallest keys per query, ascending: int64 [Q,k] (and the float32 distances, NaN as the canonical NaN).  Works on fp64
    distances too: they are ordered by value with ties to the lowest index."""
    d = np.asarray(d)
    if d.dtype == np.float64:
        dd = d.copy()
        if exclude is not None:
            for i, e in enumerate(np.asarray(exclude).reshape(-1)):
                if 0 <= e < d.shape[1]:
                    dd[i, e] = np.inf
        idx = np.argsort(dd, axis=-1, kind='stable')[:, :k]
        return (idx, np.take_along_axis(dd, idx, -1)) if return_dist else idx
    ks = np.sort(keys(d, exclude), axis=-1)[:, :k]
    idx = (ks & np.uint64(0xFFFFFFFF)).astype(np.int64)
    dist = (ks >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return (idx, dist) if return_dist else idx


# ------------------------------------------------------------------------------------------------ inputs
def codebook(K, D, seed):
    """[K,D] float32 ~ N(0,1): one embedding per row (the kernel takes its transpose, feature-major)"""
    return np.random.default_rng(seed).standard_normal((K, D)).astype(np.float32)


def lattice_codebook():
    """K = 5, D = 2 on an integer lattice: squared distances are small integers, exact ties everywhere"""
    return np.array([[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def tables(K, D, seed):
    """(E [K,D], table32_literal(E), table64(E)) of ``codebook(K, D, seed)`` (K = 5, D = 2: the lattice), computed once per process
    and read-only"""
    E = lattice_codebook() if (K, D) == (5, 2) else codebook(K, D, seed)
    out = (E, table32_literal(E), table64(E))
    for a in out:
        a.setflags(write=False)
    return out


def code_maps(n, t, K, seed):
    """int32 [n,t*t] uniform over [0, K)"""
    return np.random.default_rng(seed).integers(0, K, size=(n, t * t), dtype=np.int32)


def planted_replaced(db, rows, r, K, seed):
    """(a) query j = bank row rows[j] with r[j] tokens (r an int or one per query) replaced by random codes"""
    g = np.random.default_rng(seed)
    rows = np.asarray(rows)
    rs = np.broadcast_to(np.asarray(r), rows.shape)
    q = np.array(db[rows], copy=True)
    for j in range(len(rows)):
        at = g.choice(q.shape[1], size=int(rs[j]), replace=False)
        q[j, at] = g.integers(0, K, size=int(rs[j]))
    return q.astype(np.int32)


def planted_shifted(db, rows, t, K, seed):
    """(b) query j = bank row rows[j] shifted one token column to the right, the vacated first column random"""
    g = np.random.default_rng(seed)
    m = np.asarray(db)[np.asarray(rows)].reshape(-1, t, t)
    q = np.empty_like(m)
    q[:, :, 1:] = m[:, :, :-1]
    q[:, :, 0] = g.integers(0, K, size=(m.shape[0], t))
    return q.reshape(-1, t * t).astype(np.int32)


def rank_agreement(d32, d64, k, exclude=None):
    """the rank comparison of a float32 distance matrix with the fp64 one: tol = 4 x the largest |d32 - d64| over every query's fp64
    top-(k + 1); a query is exempt from the exact index comparison when two of its first k + 1 fp64 distances are within 2 tol.
    -> (tol, exempt bool [Q], agree bool [Q]: the float32 index list equals the fp64 one)"""
    n = min(k + 1, d64.shape[1] - (exclude is not None))
    top64, first = top_rows(d64, n, exclude, return_dist=True)
    err = np.abs(np.take_along_axis(np.asarray(d32, dtype=np.float64), top64, -1) - first)
    tol = 4 * float(err.max())
    exempt = (np.diff(first, axis=-1) <= 2 * tol).any(-1)
    agree = (top_rows(np.asarray(d32, dtype=np.float32), k, exclude) == top64[:, :k]).all(-1)
    return tol, exempt, agree
