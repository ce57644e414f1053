"""time many-views-from-one-context rendering (viewformer_amd/render.py) against the route the package offered before it:
``generate_batch_predictions`` on contexts replicated once per query view, with dummy target frames.  Full-size models of bench.py, both
arms ('mixed': fp32-equivalent encoder, bf16 transformer and decoder; 'f32'), C context views and N query views for each of B scenes:
C = 6 with (B, N) = (1, 1), (1, 128), (16, 8); C = 19 with (1, 32).  In ONE process, the two routes taking turns, every shape warmed first,
device events around calls that end in a synchronise, enough calls per window that a window is not a fraction of a second; median, min and
max of the windows.  The renderer is timed whole (set_context + render: encode, prefill, queries, decode) and, separately, render alone on
a context that is already set (an orbit's later calls).  Next to the times: the encoder passes, transformer view-rows and decoder passes
each route performs, counted from the shapes.  Plain lines, then one JSON line.  ``--only arm:C:B:N`` runs one shape (profiling).

The route being compared with needs no localization head (a model without one discards the target's codes), so both are timed on a model
without it: with the head, the evaluator's route additionally runs its LOC view."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models                                                                     # noqa: E402
from viewformer_amd.evaluate import generate_batch_predictions                                      # noqa: E402
from viewformer_amd.render import ViewRenderer                                                      # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

SHAPES = [(6, 1, 1), (6, 1, 128), (6, 16, 8), (19, 1, 32)]
MIN_WINDOW_MS = 400.0
WINDOWS = 5


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
    """what each route performs, from the shapes alone"""
    return dict(parent=dict(encodes=B * N * (C + 1), transformer_view_rows=B * N * (C + 1), decodes=B * N),
                renderer=dict(encodes=B * C, transformer_view_rows=B * (C + N), decodes=B * N),
                render_only=dict(encodes=0, transformer_view_rows=B * N, decodes=B * N))


def run_shape(dev, arm, vq, tr, C, B, N, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    ctx_f, ctx_c, q_c = frames[:, :C].contiguous(), cams[:, :C].contiguous(), cams[:, C:].contiguous()
    dummy = torch.zeros_like(ctx_f[:, :1])
    img = torch.cat([ctx_f, dummy], 1)[:, None].expand(B, N, C + 1, *ctx_f.shape[2:]).reshape(B * N, C + 1, *ctx_f.shape[2:]).contiguous()
    cam = torch.cat([ctx_c[:, None].expand(B, N, C, 7), q_c[:, :, None]], 2).reshape(B * N, C + 1, 7).contiguous()
    keep = {}
    r = ViewRenderer(tr, vq).set_context(images=ctx_f, cameras=ctx_c)

    def parent():
        keep['p'] = generate_batch_predictions(tr, vq, img, cam)['generated_images']

    def renderer():
        keep['r'] = ViewRenderer(tr, vq).set_context(images=ctx_f, cameras=ctx_c).render(q_c)['generated_images']

    def render_only():
        keep['o'] = r.render(q_c)['generated_images']
    t, calls = alternate({'parent': parent, 'renderer': renderer, 'render_only': render_only}, windows)
    res = {k: summary(v, calls[k]) for k, v in t.items()}
    views = B * N
    res['views'] = views
    res['work'] = work(C, B, N)
    res['speedup_renderer'] = round(res['parent']['median_ms'] / res['renderer']['median_ms'], 2)
    res['speedup_render_only'] = round(res['parent']['median_ms'] / res['render_only']['median_ms'], 2)
    res['same_pictures'] = round(float((keep['p'].view_as(keep['r']) == keep['r']).flatten(2).all(-1).float().mean()), 4)
    w = res['work']
    print(f'{arm:5s} C={C:2d} B={B:2d} N={N:3d}: parent {res["parent"]["median_ms"]:9.2f} ms ({res["parent"]["median_ms"] / views:7.3f} ms/view)  '
          f'renderer {res["renderer"]["median_ms"]:8.2f} ms ({res["renderer"]["median_ms"] / views:7.3f} ms/view, x{res["speedup_renderer"]})  '
          f'render alone {res["render_only"]["median_ms"]:8.2f} ms (x{res["speedup_render_only"]})')
    print(f'      spread [min..max] parent {res["parent"]["min_ms"]}..{res["parent"]["max_ms"]}  renderer {res["renderer"]["min_ms"]}..{res["renderer"]["max_ms"]}  '
          f'render alone {res["render_only"]["min_ms"]}..{res["render_only"]["max_ms"]}  ({windows} windows of {calls["parent"]} / {calls["renderer"]} / {calls["render_only"]} calls)')
    print(f'      work parent: {w["parent"]["encodes"]} encodes, {w["parent"]["transformer_view_rows"]} transformer views, {w["parent"]["decodes"]} decodes;  '
          f'renderer: {w["renderer"]["encodes"]} / {w["renderer"]["transformer_view_rows"]} / {w["renderer"]["decodes"]};  '
          f'views with identical pictures: {res["same_pictures"]}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None, help='arm:C:B:N — one shape, renderer route only, few windows (for a profiler run)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    if args.only:
        arm, C, B, N = args.only.split(':')
        C, B, N = int(C), int(B), int(N)
        vq, tr, _ = build_models(dev, False, arm, 'x3h', sequence_size=C + 1)
        frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
        frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
        for _ in range(4):
            ViewRenderer(tr, vq).set_context(images=frames[:, :C], cameras=cams[:, :C]).render(cams[:, C:])
        torch.cuda.synchronize()
        return
    for arm in ('mixed', 'f32'):
        for C in sorted({s[0] for s in SHAPES}):
            vq, tr, _ = build_models(dev, False, arm, 'x3h', sequence_size=C + 1)
            for c, B, N in SHAPES:
                if c == C:
                    out[f'{arm}_C{C}_B{B}_N{N}'] = run_shape(dev, arm, vq, tr, C, B, N)
            del vq, tr
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
