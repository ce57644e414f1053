"""time the mean view of a camera (ViewRenderer.render_mean -> MIGT.expect_from_context -> csrc/mix_rows.hip, ONE decode) against the
arg-max view and against what a user had to write before it: S samples, S decodes and an average of the images.  Full-size models of
bench.py, the 'mixed' arm (bf16 transformer), (C, B, N) = (6, 1, 1), (6, 1, 128), (6, 16, 8), decoder included.  All routes in ONE
process, taking turns, every shape warmed first, device events around calls that end in a synchronise, enough calls per window that a
window is not a fraction of a second (DESIGN.md §6.16's method); median, min and max of the windows:
  render    ``render``: the arg-max view (fused arg-max head, one decode per view)
  mean      ``render_mean()``: T = 1, no filter — every code of every token is kept, no tile of the codebook is skipped
  mean_p    ``render_mean(top_p=0.9)``: the nucleus — the row kernel walks only the code tiles some row of its workgroup keeps
  sample8   ``sample(n_samples=8)`` and the mean of the 8 decoded images per view: 8 decodes per view, still a noisy estimate
  mix       the ``ops.mix_rows`` launch alone on the shape's logits, T = 1 / top_p = 0.9
Plain lines, then one JSON line; ``--out FILE`` also writes the plain lines there (profiles/mean_views.txt), in front of
the PSNR record that file holds, which is kept."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models                                                                     # noqa: E402
from viewformer_amd import ops                                                                      # noqa: E402
from viewformer_amd.render import ViewRenderer, query_poses                                         # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

SHAPES = [(6, 1, 1), (6, 1, 128), (6, 16, 8)]
S = 8
MIN_WINDOW_MS = 400.0
WINDOWS = 5
LINES = []
RECORD_MARK = 'PSNR of the arg-max view'          # profiles/mean_views.txt: from this line on the file is not this tool's


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


def run_shape(dev, arm, vq, tr, C, B, N, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    t, nE = tr.config.token_image_size, tr.config.n_embeddings
    r = ViewRenderer(tr, vq).set_context(images=frames[:, :C].contiguous(), cameras=cams[:, :C].contiguous())
    q = cams[:, C:].contiguous()
    E = vq.codebook_embedding()
    D, rows = E.shape[0], B * N * t * t
    lg = torch.cat([tr.generate_from_context(r.cache, query_poses(q, r.transform)[:, a:b], codes_only=False)
                    for a, b, _ in r._chunks(N, None, None)], 1).reshape(rows, nE).contiguous()
    keep = {}

    def render():
        keep['render'] = r.render(q)['generated_images']

    def mean():
        keep['mean'] = r.render_mean(q)

    def mean_p():
        keep['mean_p'] = r.render_mean(q, top_p=0.9)

    def sample8():
        keep['sample8'] = r.sample(q, n_samples=S, seed=1)['generated_images'].float().mean(2)

    def mix():
        keep['mix'] = ops.mix_rows(lg, rows, nE, E, D)['out']

    def mix_p():
        keep['mix_p'] = ops.mix_rows(lg, rows, nE, E, D, top_p=0.9)['out']
    tms, calls = alternate(dict(render=render, mean=mean, mean_p=mean_p, sample8=sample8, mix=mix, mix_p=mix_p), windows)
    res = {k: summary(v, calls[k]) for k, v in tms.items()}
    res['rows'] = rows
    res['kept_mean_top_p'] = round(float(keep['mean_p']['kept'].float().mean()), 2)
    res['mean_over_render'] = round(res['mean']['median_ms'] / res['render']['median_ms'], 3)
    res['sample8_over_mean'] = round(res['sample8']['median_ms'] / res['mean']['median_ms'], 3)
    m = {k: res[k]['median_ms'] for k in tms}
    say(f'{arm:5s} C={C:2d} B={B:2d} N={N:3d}: render {m["render"]:9.3f} ms  mean {m["mean"]:9.3f} ms  mean top_p=0.9 {m["mean_p"]:9.3f} ms  '
        f'sample x{S} + average {m["sample8"]:9.3f} ms  (mean / render {res["mean_over_render"]}, sample8 / mean {res["sample8_over_mean"]})')
    say(f'      mix_rows alone on {rows} rows x {nE} codes x {D} features: T=1 {m["mix"]:8.3f} ms  top_p=0.9 {m["mix_p"]:8.3f} ms '
        f'(codes kept per token at top_p=0.9: {res["kept_mean_top_p"]})')
    say('      spread [min..max] ' + '  '.join(f'{k} {res[k]["min_ms"]}..{res[k]["max_ms"]}' for k in tms)
        + f'  ({windows} windows of ' + ' / '.join(str(calls[k]) for k in tms) + ' calls)')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arms', default='mixed')
    ap.add_argument('--windows', type=int, default=WINDOWS)
    ap.add_argument('--out', default=None, help='also write the plain lines to this file')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    for arm in args.arms.split(','):
        for C in sorted({s[0] for s in SHAPES}):
            vq, tr, _ = build_models(dev, True, arm, 'x3h', sequence_size=C + 1)
            for c, B, N in SHAPES:
                if c == C:
                    out[f'{arm}_C{C}_B{B}_N{N}'] = run_shape(dev, arm, vq, tr, C, B, N, args.windows)
            del vq, tr
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.out:
        keep = ''
        if os.path.exists(args.out):                      # what follows the times in the file (the PSNR record) stays
            with open(args.out) as f:
                old = f.read()
            at = old.find(RECORD_MARK)
            keep = old[at:] if at >= 0 else ''
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n' + ('\n' + keep if keep else ''))


if __name__ == '__main__':
    main()
