"""time "the view from 1, 2, ..., C context photos" (viewformer_amd/render.py) two ways:
  (a) what a user does without per-query context lengths: one ``set_context(first c views)`` + ``render`` per size c;
  (b) one ``set_context`` + ``sweep``: one encode and one prefill of the C views, one ``render`` over all sizes laid out size-major.
Sizes 1 ... C in both (size 0, no context photo, cannot be asked the first way at all; (b) with 0 ... C is timed as well).  Full-size models
of bench.py, both arms ('mixed': fp32-equivalent encoder, bf16 transformer and decoder; 'f32'), C = 6 with (B, N) = (1, 1), (1, 32), (16, 4),
C = 19 with (1, 8).  Also, at fixed total work, ``render`` on a context that is set with 2N views per scene of lengths 0 and C sorted
(N views of 0, then N of C) against the same lengths interleaved (0, C, 0, C, ...): what a mixed attention group costs.  In ONE process, the
routes taking turns, every route warmed first, device events around calls that end in a synchronise, windows of at least 0.4 s; median,
min and max of the windows.  Next to the times: the encoder passes, prefilled context views, query views and decoder passes each route
performs, counted from the shapes.  Plain lines, then one JSON line; the same text goes to ``--out`` (default profiles/context_sweep.txt)."""
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
from viewformer_amd.render import ViewRenderer                                                      # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

SHAPES = [(6, 1, 1), (6, 1, 32), (6, 16, 4), (19, 1, 8)]
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


def work(C, B, N):
    """what each route performs for the sizes 1 ... C, from the shapes alone"""
    tri = C * (C + 1) // 2
    return dict(per_size=dict(encodes=B * tri, prefilled_views=B * tri, query_views=B * N * C, decodes=B * N * C, set_context_calls=C),
                sweep=dict(encodes=B * C, prefilled_views=B * C, query_views=B * N * C, decodes=B * N * C, set_context_calls=1))


def run_shape(dev, arm, vq, tr, C, B, N, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    ctx_f, ctx_c, q_c = frames[:, :C].contiguous(), cams[:, :C].contiguous(), cams[:, C:].contiguous()
    sizes = list(range(1, C + 1))
    keep = {}
    r = ViewRenderer(tr, vq).set_context(images=ctx_f, cameras=ctx_c)
    q2 = torch.cat([q_c, q_c], 1)                                                                   # 2N views: N of length 0, N of length C
    sorted_len = np.repeat(np.array([0, C], dtype=np.int32), N).reshape(1, 2 * N).repeat(B, 0)
    mixed_len = np.tile(np.array([0, C], dtype=np.int32), N).reshape(1, 2 * N).repeat(B, 0)

    def per_size():
        keep['a'] = torch.stack([ViewRenderer(tr, vq).set_context(images=ctx_f[:, :c], cameras=ctx_c[:, :c]).render(q_c)['generated_images']
                                 for c in sizes], 2)

    def sweep():
        keep['b'] = ViewRenderer(tr, vq).set_context(images=ctx_f, cameras=ctx_c).sweep(q_c, sizes=sizes)['generated_images']

    def sweep_from_0():
        keep['b0'] = ViewRenderer(tr, vq).set_context(images=ctx_f, cameras=ctx_c).sweep(q_c)['generated_images']

    def lengths_sorted():
        keep['s'] = r.render(q2, n_context=sorted_len)['generated_images']

    def lengths_interleaved():
        keep['i'] = r.render(q2, n_context=mixed_len)['generated_images']
    t, calls = alternate(dict(per_size=per_size, sweep=sweep, sweep_from_0=sweep_from_0, lengths_sorted=lengths_sorted,
                              lengths_interleaved=lengths_interleaved), windows)
    res = {k: summary(v, calls[k]) for k, v in t.items()}
    res['work'] = work(C, B, N)
    res['per_size_over_sweep'] = round(res['per_size']['median_ms'] / res['sweep']['median_ms'], 2)
    res['interleaved_over_sorted'] = round(res['lengths_interleaved']['median_ms'] / res['lengths_sorted']['median_ms'], 3)
    res['same_pictures'] = round(float((keep['a'] == keep['b']).flatten(3).all(-1).float().mean()), 4)
    w = res['work']
    m = lambda k: res[k]['median_ms']
    say(f'{arm:5s} C={C:2d} B={B:2d} N={N:3d}: (a) per size {m("per_size"):9.2f} ms  (b) sweep {m("sweep"):9.2f} ms  (a)/(b) x{res["per_size_over_sweep"]}  '
        f'sweep 0..C {m("sweep_from_0"):9.2f} ms;  2N views, lengths sorted {m("lengths_sorted"):8.2f} ms, interleaved {m("lengths_interleaved"):8.2f} ms '
        f'(x{res["interleaved_over_sorted"]})')
    say('      spread [min..max] ' + '  '.join(f'{k} {res[k]["min_ms"]}..{res[k]["max_ms"]} ({calls[k]} calls)' for k in t) + f'  ({windows} windows)')
    say(f'      work (a): {w["per_size"]["encodes"]} encodes, {w["per_size"]["prefilled_views"]} prefilled views, {w["per_size"]["query_views"]} query views, '
        f'{w["per_size"]["decodes"]} decodes, {C} set_context;  (b): {w["sweep"]["encodes"]} / {w["sweep"]["prefilled_views"]} / {w["sweep"]["query_views"]} / '
        f'{w["sweep"]["decodes"]}, 1 set_context;  (camera, size) pairs with identical pictures: {res["same_pictures"]}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'context_sweep.txt'))
    ap.add_argument('--windows', type=int, default=WINDOWS)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    say(f'context-size sweep, {torch.cuda.get_device_name(0)}: ms per call, median of {args.windows} windows >= {MIN_WINDOW_MS:.0f} ms, routes alternating')
    for arm in ('mixed', 'f32'):
        for C in sorted({s[0] for s in SHAPES}):
            vq, tr, _ = build_models(dev, False, arm, 'x3h', sequence_size=C + 1)
            for c, B, N in SHAPES:
                if c == C:
                    out[f'{arm}_C{C}_B{B}_N{N}'] = run_shape(dev, arm, vq, tr, C, B, N, args.windows)
            del vq, tr
            torch.cuda.empty_cache()
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(_lines) + '\n')


if __name__ == '__main__':
    main()
