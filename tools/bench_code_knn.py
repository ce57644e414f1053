"""time the image retrieval on VQ codes (csrc/code_knn.hip) at the 7-Scenes sizes: a codebook of K = 1024 codes (D = 256), code maps
of t = 8, a bank of N in {1 000, 7 000} frames, Q in {1, 128} queries per call, k = 19, window in {0, 1, 7}.  Three routes in ONE
process, taking turns inside every round, device events around runs of calls that end in a synchronise, every shape warmed first,
medians of 5 windows:
  (a) the table build, ops.codebook_distances (once per set of weights in use: VQGAN.code_distances keeps it);
  (b) ops.code_knn;
  (c) the same search written in torch, table[q[:, None, :], db[None, :, :]].sum(-1).topk(k, largest=False) — window = 0 only: the
      windowed minimum has no torch form that fits in memory at these sizes.
Plain lines, then one JSON line.  The torch route is the yardstick; no ratio is promised and nothing asserts a speed."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viewformer_amd import ops                                                                      # noqa: E402

K, D, T, TOP = 1024, 256, 8, 19
ROUNDS = 5


def timed_ms(fn):
    """one call between device events, ending in a synchronise"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, rounds, warmup=1):
    """{name: [ms per call]} with the candidates taking turns inside every round"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed_ms(fn))
    return out


def main():
    dev = torch.device('cuda:0')
    g = np.random.default_rng(0)
    E = torch.from_numpy(g.standard_normal((D, K)).astype(np.float32)).to(dev)                      # feature-major, as VQGAN._E
    table = ops.codebook_distances(E, D, K)
    out = dict(K=K, D=D, t=T, k=TOP, rounds=ROUNDS, cases={})
    for N in (1000, 7000):
        db = torch.from_numpy(g.integers(0, K, size=(N, T * T), dtype=np.int32)).to(dev)
        for Q in (1, 128):
            # queries: bank rows with a quarter of their tokens replaced (planted neighbours, as a retrieval query has)
            qs = db[torch.from_numpy(g.integers(0, N, size=Q)).to(dev)].clone()
            mask = torch.from_numpy(g.random((Q, T * T)) < 0.25).to(dev)
            qs[mask] = torch.from_numpy(g.integers(0, K, size=int(mask.sum()), dtype=np.int32)).to(dev)
            dbl, ql = db.long(), qs.long()
            for window in (0, 1, 7):
                reps = 20 if window < 7 else 5
                keep = {}

                def build():
                    for _ in range(reps):
                        keep['table'] = ops.codebook_distances(E, D, K)

                def kernel():
                    for _ in range(reps):
                        keep['k'] = ops.code_knn(db, qs, table, TOP, window=window)

                def torch_route():
                    for _ in range(reps):
                        keep['t'] = table[ql[:, None, :], dbl[None, :, :]].sum(-1).topk(TOP, dim=-1, largest=False).indices
                fns = {'table': build, 'kernel': kernel}
                if window == 0:
                    fns['torch'] = torch_route
                t = alternate(fns, ROUNDS)
                us = {name: round(statistics.median(v) / reps * 1000, 1) for name, v in t.items()}
                case = dict(table_us=us['table'], kernel_us=us['kernel'])
                line = (f'code_knn N={N:5d} Q={Q:3d} k={TOP} window={window}: table build {us["table"]:8.1f} us  kernel {us["kernel"]:9.1f} us')
                if window == 0:
                    # the torch route sums in another order: index lists are compared, not required to agree
                    agree = float((keep['k'].long() == keep['t']).all(-1).float().mean())
                    case.update(torch_us=us['torch'], same_index_lists=round(agree, 3))
                    line += f'  torch route {us["torch"]:9.1f} us  (queries with identical index lists: {agree:.3f})'
                out['cases'][f'N{N}_Q{Q}_w{window}'] = case
                print(line + f'  [median of {ROUNDS} x {reps} calls]')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
