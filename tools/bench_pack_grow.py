"""time a roll-out of T frames — ``MIGT.rollout_from_context``, the transformer part of ``ViewRenderer.rollout`` — on context caches that
grow in place (viewformer_amd/context_cache.py):
  (a) the plain cache of ``prefill_context(capacity=C0 + T)`` (thirds V, Q, K);
  (b) the growing K/V-only cache, ``prefill_context(capacity=C0 + T, pack='kv')``: the plain cache's bits (asserted first, ``torch.equal``);
  (c) the growing e4m3 cache, ``pack='e4m3'`` (the bf16 arm only); its code maps' agreement with (a) is printed;
  (d) what a packed scene had to do before: ``unpack()`` -> roll out on the plain cache -> ``pack('e4m3')`` again.
(a), (b) and (c) roll out on an alias of one prefilled cache with room, so a call is the T steps and nothing else; (d) starts from the
tight e4m3 pack.  The decoder's pass over the maps is the same work on every route and is left out.  Full-size models of bench.py,
(C0, T, B) = (3, 16, 1), (3, 16, 16), (6, 32, 1) of profiles/rollout.txt and the library case (19, 8, 16) of profiles/pack.txt.  In ONE
process, the routes taking turns, every route warmed first, device events around calls that end in a synchronise, windows of at least
0.4 s; median, min and max of the windows.  Next to the times: the bytes of each cache at the end, from the tensor shapes
(``ContextCache.nbytes``); ``torch.cuda.max_memory_allocated`` across ``prefill_context(pack=...)`` against ``prefill_context()`` followed
by ``pack()``; and the interval between back-to-back ``vf_kv_append_split`` / ``vf_kv_append_e4m3`` launches as issued from Python
(200 launches between two events: the host's submission interval is in it, so the figure is an UPPER BOUND on the kernel's time).
Plain lines, then one JSON line; the same text goes to ``--out`` (default profiles/pack_grow.txt)."""
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

SHAPES = [(3, 16, 1), (3, 16, 16), (6, 32, 1), (19, 8, 16)]
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
    """(what ``fn`` returns, the peak of the allocator above its level before the call)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def append_us(cache, qkv_dtype, B, K, launches=200):
    """the cache's own append launch of K views per scene on layer 0, ``launches`` times back to back between two events: microseconds per
    launch AS ISSUED FROM PYTHON (ctypes call and submission included: an upper bound on the kernel's own time)"""
    src = torch.randn((B * K * 64, 3 * cache.d), device=cache.device).to(qkv_dtype)
    pos = torch.full((B,), cache.C, dtype=torch.int32, device=cache.device)       # into the slack behind the context
    fn = lambda: cache.append(0, src, K, pos)
    fn()
    torch.cuda.synchronize()
    ms = sorted(window_ms(fn, launches) for _ in range(5))
    return round(ms[2] * 1e3, 2)


def run_shape(dev, arm, tr, C0, T, B, windows=WINDOWS):
    t = tr.config.token_image_size
    g = np.random.Generator(np.random.PCG64(7))
    codes = torch.from_numpy(g.integers(0, tr.config.n_embeddings, size=(B, C0, t, t))).to(torch.int32).to(dev)
    _, cams = synthetic_scene_batch(B, C0 + T, 8, seed=7)
    poses = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0]).to(dev)
    ctx, path = poses[:, :C0].contiguous(), poses[:, C0:].contiguous()
    forms = ['plain', 'kv'] + (['e4m3'] if tr.precision == 'bf16' else [])
    peaks, base = {}, {}
    for f in forms:
        if f == 'plain':
            base[f], peaks['plain'] = peak_bytes(lambda: tr.prefill_context(codes, ctx, capacity=C0 + T))
        else:
            base[f], peaks[f + '_direct'] = peak_bytes(lambda: tr.prefill_context(codes, ctx, capacity=C0 + T, pack=f))
            _, peaks[f + '_prefill_then_pack'] = peak_bytes(lambda: tr.prefill_context(codes, ctx).pack(None if f == 'kv' else f, room=T))
    keep, last = {}, {}

    def route(name):
        def fn():
            out = tr.rollout_from_context(base[name].alias(), path)
            keep[name], last[name] = out['codes'], out['cache']
        return fn
    fns = {f: route(f) for f in forms}
    if 'e4m3' in forms:
        tight = tr.prefill_context(codes, ctx).pack('e4m3')

        def round_trip():
            out = tr.rollout_from_context(tight.unpack(), path)
            keep['unpack_rollout_pack'], last['unpack_rollout_pack'] = out['codes'], out['cache'].pack('e4m3')
        fns['unpack_rollout_pack'] = round_trip
    for fn in fns.values():
        fn()
    assert torch.equal(keep['plain'], keep['kv']), 'the growing K/V-only cache rolled out different code maps'
    agree = None if 'e4m3' not in forms else round((keep['e4m3'] == keep['plain']).float().mean().item(), 4)
    t_ms, calls = alternate(fns, windows)
    res = {k: summary(v, calls[k]) for k, v in t_ms.items()}
    res['cache_bytes_at_the_end'] = {k: c.nbytes() for k, c in last.items()}
    res['prefill_peak_bytes'] = peaks
    res['codes_agreeing_with_plain'] = agree
    qdt = base['plain'].kv[0].dtype
    res['append_us'] = {f'{f}_K{K}': append_us(base[f], qdt, B, K) for f in forms for K in (1, 2)}
    m = lambda k: res[k]['median_ms']
    mb = lambda x: f'{x / 1e6:.1f} MB'
    say(f'{arm:5s} C0={C0:2d} T={T:2d} B={B:2d}: ' + '  '.join(f'{k} {m(k):9.3f} ms' for k in fns)
        + '  plain/' + '  plain/'.join(f'{k} x{m("plain") / m(k):.3f}' for k in fns if k != 'plain')
        + ('' if agree is None else f'  e4m3 codes equal to plain: {agree}'))
    say('      spread [min..max] ' + '  '.join(f'{k} {res[k]["min_ms"]}..{res[k]["max_ms"]} ({calls[k]} calls)' for k in t_ms) + f'  ({windows} windows)')
    say('      cache bytes at the end: ' + '  '.join(f'{k} {mb(v)}' for k, v in res['cache_bytes_at_the_end'].items())
        + ';  peak allocated across the prefill: ' + '  '.join(f'{k} {mb(v)}' for k, v in peaks.items()))
    say('      append per back-to-back launch as issued from Python (us): ' + '  '.join(f'{k} {v}' for k, v in res['append_us'].items()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pack_grow.txt'))
    ap.add_argument('--windows', type=int, default=WINDOWS)
    ap.add_argument('--arms', default='mixed,f32')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    say(f'a roll-out of T frames on a plain, a growing K/V-only and a growing e4m3 context cache, and through unpack() -> rollout -> pack(), '
        f'{torch.cuda.get_device_name(0)}: ms per rollout_from_context (the transformer part of rollout), median of {args.windows} windows >= '
        f'{MIN_WINDOW_MS:.0f} ms, routes alternating; cache bytes from the shapes')
    for arm in args.arms.split(','):
        _, tr, _ = build_models(dev, False, arm, 'x3h', sequence_size=max(c + t for c, t, _ in SHAPES) + 1)
        for C0, T, B in SHAPES:
            out[f'{arm}_C{C0}_T{T}_B{B}'] = run_shape(dev, arm, tr, C0, T, B, args.windows)
        del tr
        torch.cuda.empty_cache()
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(_lines) + '\n')


if __name__ == '__main__':
    main()
