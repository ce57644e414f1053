"""time the drawing of S code maps per query view from one context of C photographs (MIGT.sample_from_context -> csrc/sample_rows.hip)
against what a user had to write before it.  Full-size models of bench.py, the 'mixed' arm (bf16 transformer), (C, B, N) = (6, 1, 1),
(6, 1, 128), (6, 16, 8) at S = 1 and S = 8, top_k = 64 at temperature 1 in both sampling routes; the decoder is left out (the same S
decodes follow either route).  Three routes in ONE process, taking turns, every shape warmed first, device events around calls that end
in a synchronise, enough calls per window that a window is not a fraction of a second; median, min and max of the windows:
  torch     ``generate_from_context(codes_only=False)`` + ``torch.topk`` mask + ``torch.softmax`` + ``torch.multinomial(S)``
  sample    ``sample_from_context(n_samples=S, top_k=64)``: the logits, then ONE row kernel (filters, S draws, their log-probabilities)
            and the in-order log-likelihood chain
  greedy    ``generate_from_context`` (the fused arg-max head), for scale
The torch route returns codes only — no log-probabilities, and its draws depend on torch's generator state and launch geometry; it is the
yardstick, not an alternative to ship.  Plain lines, then one JSON line; ``--out FILE`` also writes the plain lines there
(profiles/sample_views.txt)."""
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
SAMPLES = (1, 8)
TOP_K = 64
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


def run_shape(dev, arm, vq, tr, C, B, N, S, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    t, nE = tr.config.token_image_size, tr.config.n_embeddings
    r = ViewRenderer(tr, vq).set_context(images=frames[:, :C].contiguous(), cameras=cams[:, :C].contiguous())
    poses = query_poses(cams[:, C:].contiguous(), r.transform)
    keep = {}

    def torch_route():
        parts = []
        for a, b in plan_view_chunks(N, B):
            lg = tr.generate_from_context(r.cache, poses[:, a:b], codes_only=False).view(-1, nE)
            kth = torch.topk(lg, TOP_K, -1).values[:, -1:]
            p = torch.softmax(lg.masked_fill(lg < kth, float('-inf')), -1)
            parts.append(torch.multinomial(p, S, replacement=True).view(B, b - a, t * t, S))
        keep['torch'] = torch.cat(parts, 1) if len(parts) > 1 else parts[0]

    def sample():
        parts = [tr.sample_from_context(r.cache, poses[:, a:b], n_samples=S, top_k=TOP_K, seed=1, view0=a) for a, b in plan_view_chunks(N, B)]
        keep['sample'] = parts[0]['codes'] if len(parts) == 1 else torch.cat([p['codes'] for p in parts], 1)

    def greedy():
        parts = [tr.generate_from_context(r.cache, poses[:, a:b]) for a, b in plan_view_chunks(N, B)]
        keep['greedy'] = parts[0] if len(parts) == 1 else torch.cat(parts, 1)
    tms, calls = alternate({'torch': torch_route, 'sample': sample, 'greedy': greedy}, windows)
    res = {k: summary(v, calls[k]) for k, v in tms.items()}
    rows = B * N * t * t
    res['rows'] = rows
    res['torch_over_sample'] = round(res['torch']['median_ms'] / res['sample']['median_ms'], 3)
    res['sample_over_greedy'] = round(res['sample']['median_ms'] / res['greedy']['median_ms'], 3)
    # both sampling routes draw from the same top-64 sets: the share of draws that are the greedy code, as a sanity figure
    g = keep['greedy'].reshape(B, N, t * t)
    res['share_greedy_torch'] = round(float((keep['torch'] == g[..., None]).float().mean()), 4)
    res['share_greedy_sample'] = round(float((keep['sample'].reshape(B, N, S, t * t) == g[:, :, None]).float().mean()), 4)
    say(f'{arm:5s} C={C:2d} B={B:2d} N={N:3d} S={S}: torch {res["torch"]["median_ms"]:8.3f} ms  sample {res["sample"]["median_ms"]:8.3f} ms '
        f'(torch / sample {res["torch_over_sample"]})  greedy {res["greedy"]["median_ms"]:8.3f} ms (sample / greedy {res["sample_over_greedy"]})')
    say(f'      spread [min..max] torch {res["torch"]["min_ms"]}..{res["torch"]["max_ms"]}  sample {res["sample"]["min_ms"]}..{res["sample"]["max_ms"]}  '
        f'greedy {res["greedy"]["min_ms"]}..{res["greedy"]["max_ms"]}  ({windows} windows of {calls["torch"]} / {calls["sample"]} / {calls["greedy"]} calls)')
    say(f'      {rows} token rows x {nE} codes; share of draws equal to the greedy code: torch {res["share_greedy_torch"]}, sample {res["share_greedy_sample"]}')
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
                for S in SAMPLES:
                    if c == C:
                        out[f'{arm}_C{C}_B{B}_N{N}_S{S}'] = run_shape(dev, arm, vq, tr, C, B, N, S, args.windows)
            del vq, tr
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
