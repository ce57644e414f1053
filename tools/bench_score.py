"""time the scoring of N photos at N cameras against one context of C photographs (viewformer_amd/render.py: ViewRenderer.score ->
MIGT.score_from_context) against the only route the package offered before it.  Full-size models of bench.py, the 'mixed' arm (bf16
transformer: the arm the fused head serves; ``--arms mixed,f32`` adds the fp32 arm, where routes b and c are the same launches),
(C, B, N) = (6, 1, 1), (6, 1, 128), (6, 16, 8).  The photos' codes are encoded beforehand (the encoder pass is the same in every route).
Three routes in ONE process, taking turns, every shape warmed first, device events around calls that end in a synchronise, enough calls
per window that a window is not a fraction of a second; median, min and max of the windows:
  logits    ``generate_from_context(codes_only=False)`` + ``torch.log_softmax`` + gather at the codes + sum over a view's tokens
  fused     ``score_from_context(fused=True)``: the soft-max statistics in the LM head's epilogue (csrc/lmhead_score.hip)
  unfused   ``score_from_context(fused=False)``: the logits, then the row kernel on them
(fused and unfused go through ``ViewRenderer.score``, which prepares poses and targets per call; logits is handed prepared poses: compare
fused with unfused for the kernels, either with logits for the whole call.)  Next to the times: the bytes of logits each route writes, counted from the shapes.  Plain lines, then one JSON line; ``--out FILE`` also
writes the plain lines there (profiles/score_views.txt)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models                                                                     # noqa: E402
from viewformer_amd.render import ViewRenderer, plan_view_chunks, query_poses                       # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

SHAPES = [(6, 1, 1), (6, 1, 128), (6, 16, 8)]
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


def logits_bytes(rows, nE):
    """bytes of [rows][nE] fp32 logits each route writes per call: the GEMM's store, and log_softmax's store of as much again"""
    return dict(logits=2 * rows * nE * 4, fused=0, unfused=rows * nE * 4)


def run_shape(dev, arm, vq, tr, C, B, N, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    t, nE = tr.config.token_image_size, tr.config.n_embeddings
    r = ViewRenderer(tr, vq).set_context(images=frames[:, :C].contiguous(), cameras=cams[:, :C].contiguous())
    r_unfused = ViewRenderer(tr, vq)
    r_unfused.cache, r_unfused.transform, r_unfused.context_codes = r.cache, r.transform, r.context_codes      # the same context, set once
    r.fused_score, r_unfused.fused_score = True, False
    q = cams[:, C:].contiguous()
    codes = vq.encode(frames[:, C:].reshape(B * N, 128, 128, 3))[-1].to(torch.int32).view(B, N, t, t)
    poses = query_poses(q, r.transform)
    gather_at = codes.long().unsqueeze(-1)
    keep = {}

    def logits():
        parts = []
        for a, b in plan_view_chunks(N, B):
            lg = tr.generate_from_context(r.cache, poses[:, a:b], codes_only=False)
            parts.append(torch.log_softmax(lg, -1).gather(-1, gather_at[:, a:b])[..., 0])
        tlp = torch.cat(parts, 1) if len(parts) > 1 else parts[0]
        keep['logits'] = (tlp, tlp.sum((2, 3)))

    def fused():
        o = r.score(q, codes=codes)
        keep['fused'] = (o['token_log_prob'], o['log_likelihood'])

    def unfused():
        o = r_unfused.score(q, codes=codes)
        keep['unfused'] = (o['token_log_prob'], o['log_likelihood'])
    tms, calls = alternate({'logits': logits, 'fused': fused, 'unfused': unfused}, windows)
    res = {k: summary(v, calls[k]) for k, v in tms.items()}
    rows = B * N * t * t
    res['rows'] = rows
    res['logits_bytes_written'] = logits_bytes(rows, nE)
    res['speedup_fused_vs_logits'] = round(res['logits']['median_ms'] / res['fused']['median_ms'], 3)
    res['unfused_over_fused'] = round(res['unfused']['median_ms'] / res['fused']['median_ms'], 3)
    res['max_log_prob_diff_fused_vs_logits'] = float((keep['fused'][0] - keep['logits'][0]).abs().max())
    res['max_log_prob_diff_fused_vs_unfused'] = float((keep['fused'][0] - keep['unfused'][0]).abs().max())
    lb = res['logits_bytes_written']
    say(f'{arm:5s} C={C:2d} B={B:2d} N={N:3d}: logits {res["logits"]["median_ms"]:8.3f} ms  fused {res["fused"]["median_ms"]:8.3f} ms '
        f'(x{res["speedup_fused_vs_logits"]})  unfused {res["unfused"]["median_ms"]:8.3f} ms (unfused / fused {res["unfused_over_fused"]})')
    say(f'      spread [min..max] logits {res["logits"]["min_ms"]}..{res["logits"]["max_ms"]}  fused {res["fused"]["min_ms"]}..{res["fused"]["max_ms"]}  '
        f'unfused {res["unfused"]["min_ms"]}..{res["unfused"]["max_ms"]}  ({windows} windows of {calls["logits"]} / {calls["fused"]} / {calls["unfused"]} calls)')
    say(f'      {rows} token rows; bytes of logits written per call: logits {lb["logits"]}, fused {lb["fused"]}, unfused {lb["unfused"]};  '
        f'largest log-probability difference fused - logits {res["max_log_prob_diff_fused_vs_logits"]:.2e}, fused - unfused '
        f'{res["max_log_prob_diff_fused_vs_unfused"]:.2e}')
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
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
