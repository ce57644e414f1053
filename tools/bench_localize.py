"""time the localization of N photos against one context of C photographs (viewformer_amd/render.py: ViewRenderer.localize) against the
strongest route the package offered before it.  Full-size models of bench.py with the localization head, both arms ('mixed': fp32-equivalent
encoder, bf16 transformer; 'f32'), (C, B, N) = (6, 1, 1), (6, 1, 128), (19, 1, 32).  Three routes in ONE process, taking turns, every shape
warmed first, device events around calls that end in a synchronise, enough calls per window that a window is not a fraction of a second;
median, min and max of the windows:
  full      the context's codes encoded beforehand; the N photos are encoded and the full pass
            ``model(dict(input_ids=[ctx, photo n], poses=ctx), last_view_logits_only=True)`` runs on the B * N replicated scenes, then
            ``reduce_cameras`` and the frame change
  fused     ``ViewRenderer.localize`` on a context that is already set, the pose head's tail as one launch (ops.pose_tail)
  unfused   the same with ``fused_tail=False``: c_proj GEMM, ``geometry.pose_head_postprocess``, ``reduce_cameras``
Next to the times: the encoder passes and transformer view-rows each route performs, counted from the shapes.  Plain lines, then one JSON
line; ``--out FILE`` also writes the plain lines there (profiles/localize_views.txt).  ``--only arm:C:B:N`` runs the fused route of one shape
(profiling)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models                                                                     # noqa: E402
from viewformer_amd import geometry                                                                 # noqa: E402
from viewformer_amd.evaluate import _frames_for_encode                                              # noqa: E402
from viewformer_amd.render import ViewRenderer, context_poses                                                      # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

SHAPES = [(6, 1, 1), (6, 1, 128), (19, 1, 32)]
MIN_WINDOW_MS = 400.0
WINDOWS = 5
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


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
    """what each route performs per call, from the shapes alone (the context's own C encodes and C views are paid once, before either)"""
    return dict(full=dict(encodes=B * N, transformer_view_rows=B * N * (C + 1)), cached=dict(encodes=B * N, transformer_view_rows=B * N),
                evaluator=dict(encodes=B * N * (C + 1), transformer_view_rows=B * N * (C + 1)))


def run_shape(dev, arm, vq, tr, C, B, N, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    ctx_f, ctx_c, photos = frames[:, :C].contiguous(), cams[:, :C].contiguous(), frames[:, C:].contiguous()
    t = tr.config.token_image_size
    keep = {}
    r_fused, r_unfused = (ViewRenderer(tr, vq).set_context(images=ctx_f, cameras=ctx_c) for _ in range(2))
    r_fused.fused_tail, r_unfused.fused_tail = True, False
    ctx_codes = r_fused.context_codes                                               # [B,C,t,t], encoded beforehand
    ctx_rep = ctx_codes[:, None].expand(B, N, C, t, t).reshape(B * N, C, t, t).contiguous()
    poses, transform = context_poses(ctx_c, tr.config.augment_poses)
    poses_rep = poses[:, None].expand(B, N, C, 7).reshape(B * N, C, 7).contiguous()

    def full():
        codes = vq.encode(_frames_for_encode(photos, vq.config.image_size))[-1].to(torch.int32).view(B * N, 1, t, t)
        out = tr(dict(input_ids=torch.cat([ctx_rep, codes], 1), poses=poses_rep), last_view_logits_only=True)
        cam = tr.reduce_cameras(out['pose_prediction'][:, -1], -2).view(B, N, 7)
        keep['full'] = geometry.from_relative_cameras(cam, transform) if transform is not None else cam

    def fused():
        keep['fused'] = r_fused.localize(images=photos)['generated_cameras']

    def unfused():
        keep['unfused'] = r_unfused.localize(images=photos)['generated_cameras']
    tms, calls = alternate({'full': full, 'fused': fused, 'unfused': unfused}, windows)
    res = {k: summary(v, calls[k]) for k, v in tms.items()}
    views = B * N
    res['views'] = views
    res['work'] = work(C, B, N)
    res['speedup_fused_vs_full'] = round(res['full']['median_ms'] / res['fused']['median_ms'], 2)
    res['fused_vs_unfused'] = round(res['unfused']['median_ms'] / res['fused']['median_ms'], 3)
    res['max_camera_diff_fused_vs_full'] = float((keep['fused'] - keep['full']).abs().max())
    res['max_camera_diff_fused_vs_unfused'] = float((keep['fused'] - keep['unfused']).abs().max())
    w = res['work']
    say(f'{arm:5s} C={C:2d} B={B:2d} N={N:3d}: full {res["full"]["median_ms"]:9.3f} ms ({res["full"]["median_ms"] / views:7.3f} ms/photo)  '
        f'fused {res["fused"]["median_ms"]:8.3f} ms ({res["fused"]["median_ms"] / views:7.3f} ms/photo, x{res["speedup_fused_vs_full"]})  '
        f'unfused {res["unfused"]["median_ms"]:8.3f} ms (unfused / fused {res["fused_vs_unfused"]})')
    say(f'      spread [min..max] full {res["full"]["min_ms"]}..{res["full"]["max_ms"]}  fused {res["fused"]["min_ms"]}..{res["fused"]["max_ms"]}  '
        f'unfused {res["unfused"]["min_ms"]}..{res["unfused"]["max_ms"]}  ({windows} windows of {calls["full"]} / {calls["fused"]} / {calls["unfused"]} calls)')
    say(f'      work per call, full: {w["full"]["encodes"]} encodes, {w["full"]["transformer_view_rows"]} transformer views;  cached: '
        f'{w["cached"]["encodes"]} / {w["cached"]["transformer_view_rows"]};  (the evaluator, re-encoding its contexts: {w["evaluator"]["encodes"]} / '
        f'{w["evaluator"]["transformer_view_rows"]});  largest camera difference fused - full {res["max_camera_diff_fused_vs_full"]:.2e}, '
        f'fused - unfused {res["max_camera_diff_fused_vs_unfused"]:.2e}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None, help='arm:C:B:N — one shape, fused route only, a few calls (for a profiler run)')
    ap.add_argument('--arms', default='mixed,f32')
    ap.add_argument('--out', default=None, help='also write the plain lines to this file')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    if args.only:
        arm, C, B, N = args.only.split(':')
        C, B, N = int(C), int(B), int(N)
        vq, tr, _ = build_models(dev, True, arm, 'x3h', sequence_size=C + 1)
        frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
        frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
        r = ViewRenderer(tr, vq).set_context(images=frames[:, :C], cameras=cams[:, :C])
        for _ in range(4):
            r.localize(images=frames[:, C:])
        torch.cuda.synchronize()
        return
    for arm in args.arms.split(','):
        for C in sorted({s[0] for s in SHAPES}):
            vq, tr, _ = build_models(dev, True, arm, 'x3h', sequence_size=C + 1)
            for c, B, N in SHAPES:
                if c == C:
                    out[f'{arm}_C{C}_B{B}_N{N}'] = run_shape(dev, arm, vq, tr, C, B, N)
            del vq, tr
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
