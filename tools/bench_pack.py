"""time the transformer part of ``render`` — ``MIGT.generate_from_context`` of N novel views per scene — on three caches of the same
context (viewformer_amd/migt.py):
  (a) the plain cache of ``prefill_context`` (thirds V, Q, K);
  (b) ``cache.pack()``: the K and V thirds only, the plain cache's bits;
  (c) ``cache.pack('e4m3')`` (the bf16 arm only): e4m3 bytes with a power-of-two scale per (scene, view, head).
(a) and (b) return the same code maps (asserted first, ``torch.equal``); (c) returns those of the dequantised cache (asserted against
``unpack()``), and its agreement with (a) is printed.  The decoder's pass over the maps is the same work on every route and is left out.
Full-size models of bench.py, both arms ('mixed': the bf16 transformer; 'f32'), (C, B, N) = (6, 1, 128), (19, 16, 8), (19, 1, 32).  In ONE
process, the routes taking turns, every route warmed first, device events around calls that end in a synchronise, windows of at least
0.4 s; median, min and max of the windows.  Next to the times: the bytes of each cache, from the tensor shapes
(``ContextCache.nbytes``).  Plain lines, then one JSON line; the same text goes to ``--out`` (default profiles/pack.txt)."""
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

SHAPES = [(6, 1, 128), (19, 16, 8), (19, 1, 32)]
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


def run_shape(dev, arm, tr, C, B, N, windows=WINDOWS):
    t = tr.config.token_image_size
    g = np.random.Generator(np.random.PCG64(7))
    codes = torch.from_numpy(g.integers(0, tr.config.n_embeddings, size=(B, C, t, t))).to(torch.int32).to(dev)
    _, cams = synthetic_scene_batch(B, C + N, 8, seed=7)
    poses = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0]).to(dev)
    ctx, query = poses[:, :C].contiguous(), poses[:, C:].contiguous()
    caches = dict(plain=tr.prefill_context(codes, ctx))
    caches['kv'] = caches['plain'].pack()
    if tr.precision == 'bf16':
        caches['e4m3'] = caches['plain'].pack('e4m3')
    keep = {}

    def route(name):
        def fn():
            keep[name] = tr.generate_from_context(caches[name], query)
        return fn
    fns = {k: route(k) for k in caches}
    for fn in fns.values():
        fn()
    assert torch.equal(keep['plain'], keep['kv']), 'the K/V-only cache generated different code maps'
    agree = None
    if 'e4m3' in caches:
        assert torch.equal(keep['e4m3'], tr.generate_from_context(caches['e4m3'].unpack(), query)), 'the e4m3 cache is not its dequantised cache'
        agree = round((keep['e4m3'] == keep['plain']).float().mean().item(), 4)
    t_ms, calls = alternate(fns, windows)
    res = {k: summary(v, calls[k]) for k, v in t_ms.items()}
    res['cache_bytes'] = {k: c.nbytes() for k, c in caches.items()}
    res['codes_agreeing_with_plain'] = agree
    m = lambda k: res[k]['median_ms']
    mb = lambda x: f'{x / 1e6:.1f} MB'
    say(f'{arm:5s} C={C:2d} B={B:2d} N={N:3d}: ' + '  '.join(f'{k} {m(k):8.3f} ms ({mb(res["cache_bytes"][k])})' for k in caches)
        + '  plain/' + '  plain/'.join(f'{k} x{m("plain") / m(k):.3f}' for k in caches if k != 'plain')
        + ('' if agree is None else f'  e4m3 codes equal to plain: {agree}'))
    say('      spread [min..max] ' + '  '.join(f'{k} {res[k]["min_ms"]}..{res[k]["max_ms"]} ({calls[k]} calls)' for k in t_ms) + f'  ({windows} windows)')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pack.txt'))
    ap.add_argument('--windows', type=int, default=WINDOWS)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    say(f'N novel views per scene from a plain, a K/V-only and an e4m3 context cache, {torch.cuda.get_device_name(0)}: ms per generate_from_context '
        f'(the transformer part of render), median of {args.windows} windows >= {MIN_WINDOW_MS:.0f} ms, routes alternating; cache bytes from the shapes')
    for arm in ('mixed', 'f32'):
        _, tr, _ = build_models(dev, False, arm, 'x3h', sequence_size=max(c for c, _, _ in SHAPES) + 1)
        for C, B, N in SHAPES:
            out[f'{arm}_C{C}_B{B}_N{N}'] = run_shape(dev, arm, tr, C, B, N, args.windows)
        del tr
        torch.cuda.empty_cache()
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(_lines) + '\n')


if __name__ == '__main__':
    main()
