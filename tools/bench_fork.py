"""time S camera-path trajectories per scene from one context (viewformer_amd/migt.py) two ways:
  (a) ``MIGT.rollout_from_context(n_samples=S)``: the context cache is replicated S times per scene, then rolled out;
  (b) the same call with ``fork=True``: the trajectories read the photographs' keys where they lie and own only their T generated views.
Both return the same code maps (asserted first, ``torch.equal``).  The transformer's roll-out alone is timed — the decoder's pass over the
S*T maps is the same work on both routes — on a context prefilled with room for the path (capacity C0 + T), so that route (a) replicates
once and never reallocates: the cheaper of its two forms.  Full-size models of bench.py, both arms ('mixed': the bf16 transformer;
'f32'), (C0, T, B, S) = (6, 8, 1, 16), (19, 4, 1, 64), (6, 16, 4, 8).  In ONE process, the routes taking turns, every route warmed first,
device events around calls that end in a synchronise, windows of at least 0.4 s; median, min and max of the windows.  Next to the times:
the bytes of cache each route allocates per call, computed from the tensor shapes, and the difference of the two routes' peak allocations
(``torch.cuda.max_memory_allocated`` over one call; activations and logits are the same on both routes and cancel) as a cross-check.
Plain lines, then one JSON line; the same text goes to ``--out`` (default profiles/fork.txt)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bench import build_models                                                                     # noqa: E402
from viewformer_amd import geometry                                                                 # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

SHAPES = [(6, 8, 1, 16), (19, 4, 1, 64), (6, 16, 4, 8)]
MIN_WINDOW_MS = 400.0
WINDOWS = 5
_lines = []


def say(line):
    print(line, flush=True)
    _lines.append(line)


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fns, windows=WINDOWS):
    """{name: [ms per call, one figure per window]}: every candidate is warmed, sized to MIN_WINDOW_MS per window, and the candidates take turns"""
    calls = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        one = window_ms(fn, 1)
        calls[k] = max(1, int(MIN_WINDOW_MS / max(one, 1e-3)) + 1)
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, calls[k]))
    return out, calls


def summary(ms, calls):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), windows=len(ms), calls_per_window=calls)


def peak_bytes(fn):
    """peak allocation of one call above what was allocated before it (the call's result is dropped before returning)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run_shape(dev, arm, tr, C0, T, B, S, windows=WINDOWS):
    t = tr.config.token_image_size
    g = np.random.Generator(np.random.PCG64(7))
    codes = torch.from_numpy(g.integers(0, tr.config.n_embeddings, size=(B, C0, t, t))).to(torch.int32).to(dev)
    _, cams = synthetic_scene_batch(B, C0 + T, 8, seed=7)
    poses = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0]).to(dev)
    ctx, path = poses[:, :C0].contiguous(), poses[:, C0:].contiguous()
    cache = tr.prefill_context(codes, ctx, capacity=C0 + T)
    kw = dict(n_samples=S, top_k=0, seed=3)
    keep = {}

    def route(name, **extra):
        def fn():
            out = tr.rollout_from_context(cache, path, **kw, **extra)
            keep[name] = out['codes']
            keep[name + '_cache'] = [tuple(x.shape) for x in out['cache'].kv]
        return fn
    replicate, fork = route('a'), route('b', fork=True)
    replicate()
    fork()
    assert torch.equal(keep['a'], keep['b']), 'the two routes rolled out different code maps'
    elem = cache.kv[0].element_size()
    by_shape = {k: sum(r * c for r, c in keep[k + '_cache']) * elem for k in ('a', 'b')}
    keep.clear()
    peaks = dict(a=peak_bytes(lambda: (replicate(), keep.clear())), b=peak_bytes(lambda: (fork(), keep.clear())))
    t_ms, calls = alternate(dict(replicate=replicate, fork=fork), windows)
    keep.clear()
    res = {k: summary(v, calls[k]) for k, v in t_ms.items()}
    res['a_over_b'] = round(res['replicate']['median_ms'] / res['fork']['median_ms'], 3)
    res['cache_bytes'] = dict(replicate=by_shape['a'], fork=by_shape['b'], views=dict(replicate=B * S * (C0 + T), fork=B * S * T, distinct=B * (C0 + S * T)))
    res['peak_bytes'] = dict(replicate=peaks['a'], fork=peaks['b'], difference=peaks['a'] - peaks['b'], difference_from_shapes=by_shape['a'] - by_shape['b'])
    m = lambda k: res[k]['median_ms']
    mb = lambda x: f'{x / 1e6:.1f} MB'
    say(f'{arm:5s} C0={C0:2d} T={T:2d} B={B} S={S:2d}: (a) replicate {m("replicate"):9.2f} ms  (b) fork {m("fork"):9.2f} ms  (a)/(b) x{res["a_over_b"]}')
    say('      spread [min..max] ' + '  '.join(f'{k} {res[k]["min_ms"]}..{res[k]["max_ms"]} ({calls[k]} calls)' for k in t_ms) + f'  ({windows} windows)')
    cb, pk = res['cache_bytes'], res['peak_bytes']
    say(f'      cache allocated per call, from the shapes: (a) {mb(cb["replicate"])} ({cb["views"]["replicate"]} views)  (b) {mb(cb["fork"])} '
        f'({cb["views"]["fork"]} views; {cb["views"]["distinct"]} distinct views with the parent\'s);  peak allocation of one call: (a) {mb(pk["replicate"])}  '
        f'(b) {mb(pk["fork"])}  difference {mb(pk["difference"])} against {mb(pk["difference_from_shapes"])} from the shapes')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'fork.txt'))
    ap.add_argument('--windows', type=int, default=WINDOWS)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    say(f'S trajectories per scene, replicated cache against forked cache, {torch.cuda.get_device_name(0)}: ms per roll-out of the transformer, '
        f'median of {args.windows} windows >= {MIN_WINDOW_MS:.0f} ms, routes alternating')
    for arm in ('mixed', 'f32'):
        _, tr, _ = build_models(dev, False, arm, 'x3h', sequence_size=max(c + t for c, t, _, _ in SHAPES) + 1)
        for C0, T, B, S in SHAPES:
            out[f'{arm}_C{C0}_T{T}_B{B}_S{S}'] = run_shape(dev, arm, tr, C0, T, B, S, args.windows)
        del tr
        torch.cuda.empty_cache()
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(_lines) + '\n')


if __name__ == '__main__':
    main()
