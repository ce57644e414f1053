"""time the matching of P photos to M cameras against one context of C photographs (viewformer_amd/render.py: ViewRenderer.match ->
MIGT.match_from_context -> csrc/match_views.hip) against the only route the package offered before it: P calls of ``ViewRenderer.score``,
each with one photo against the M cameras.  Full-size models of bench.py, the 'mixed' arm (bf16 transformer), (C, B, P, M) = (6, 1, 8, 8),
(6, 1, 64, 64), (6, 1, 7000, 16) — a handful of photos, a square problem, a scene bank's frames against a few cameras.  The photos are
seeded random code maps (encoding is the same pass in both routes and is left out; the kernel's gathers do not depend on which codes
they are, beyond the cache lines they share).  Both routes in ONE process, taking turns, every shape warmed first, device events around
calls that end in a synchronise, enough calls per window that a window is at least 400 ms; median, min and max of the windows:
  loop    for p in range(P): score(cameras, codes=photo p)       P x M query views through the transformer
  match   match(cameras, codes=photos)                            M query views, one LM head, one gather-and-sum launch
  kernel  ops.match_views alone on the M views' logits, lse and idx (what ``match`` adds to one ``score`` call of M views)
Next to the times: the query views each route runs, the bytes the kernel touches counted from the shapes, and the number of elements in
which the two routes' log-likelihoods differ (0: ``match`` has the loop's bits).  Plain lines, then one JSON line; ``--out FILE`` also
writes the plain lines there (profiles/match_views.txt)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models                                                                     # noqa: E402
from viewformer_amd import ops                                                                     # noqa: E402
from viewformer_amd.render import ViewRenderer, query_poses                                        # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

SHAPES = [(6, 1, 8, 8), (6, 1, 64, 64), (6, 1, 7000, 16)]
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
        while calls[k] > 1:                                               # back to back, short calls run faster than one call alone: size again
            took = window_ms(fn, calls[k]) * calls[k]
            if took >= MIN_WINDOW_MS:
                break
            calls[k] = int(calls[k] * 1.1 * MIN_WINDOW_MS / max(took, 1e-3)) + 1
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, calls[k]))
    return out, calls


def summary(ms, calls):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), windows=len(ms), calls_per_window=calls)


def kernel_bytes(B, M, P, L, V):
    """what one vf_match_views_f32 launch touches, from the shapes: every (camera, photo) pair reads the photo's L codes and gathers L
    logits (4 bytes each, from a view of L x V x 4 bytes that the photo tiles of that camera share), and writes two floats"""
    return dict(codes_read=B * M * P * L * 4, logits_gathered=B * M * P * L * 4, view_logits=B * M * L * V * 4, written=B * M * P * 8)


def run_shape(dev, arm, vq, tr, C, B, P, M, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C + M, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    t, nE = tr.config.token_image_size, tr.config.n_embeddings
    L = t * t
    r = ViewRenderer(tr, vq).set_context(images=frames[:, :C].contiguous(), cameras=cams[:, :C].contiguous())
    q = cams[:, C:].contiguous()
    g = np.random.Generator(np.random.PCG64(11 + P))
    codes = torch.from_numpy(g.integers(0, nE, size=(B, P, t, t)).astype(np.int32)).to(dev)
    one_photo = [codes[:, p:p + 1].contiguous() for p in range(P)]
    keep = {}

    def loop():
        keep['loop'] = torch.stack([r.score(q, codes=c)['log_likelihood'] for c in one_photo], 1)          # [B,P,M]

    def match():
        keep['match'] = r.match(q, codes=codes)['log_likelihood']

    # the kernel alone: the M views' logits and statistics as match_from_context forms them, once
    R = B * M * L
    lg = tr.generate_from_context(r.cache, query_poses(q, r.transform), codes_only=False).reshape(R, nE).contiguous()
    st = ops.logits_score(lg, R, nE, want=('idx', 'lse'))
    flat = codes.view(B, P, L)

    def kernel():
        keep['kernel'] = ops.match_views(lg, st['lse'], st['idx'], flat, B, M, P, L, nE)[0]
    tms, calls = alternate({'loop': loop, 'match': match, 'kernel': kernel}, windows)
    res = {k: summary(v, calls[k]) for k, v in tms.items()}
    res['query_views'] = dict(loop=B * P * M, match=B * M)
    res['kernel_bytes'] = kernel_bytes(B, M, P, L, nE)
    res['speedup_match_vs_loop'] = round(res['loop']['median_ms'] / res['match']['median_ms'], 2)
    res['elements_differing_match_vs_loop'] = int((keep['match'].contiguous().view(torch.int32) != keep['loop'].contiguous().view(torch.int32)).sum())
    res['elements_differing_kernel_vs_match'] = int((keep['kernel'].transpose(1, 2).contiguous().view(torch.int32)
                                                    != keep['match'].contiguous().view(torch.int32)).sum())
    kb = res['kernel_bytes']
    say(f'{arm:5s} C={C:2d} B={B:2d} P={P:4d} M={M:3d}: loop {res["loop"]["median_ms"]:10.3f} ms  match {res["match"]["median_ms"]:8.3f} ms '
        f'(x{res["speedup_match_vs_loop"]})  kernel alone {res["kernel"]["median_ms"]:8.4f} ms')
    say(f'      spread [min..max] loop {res["loop"]["min_ms"]}..{res["loop"]["max_ms"]}  match {res["match"]["min_ms"]}..{res["match"]["max_ms"]}  '
        f'kernel {res["kernel"]["min_ms"]}..{res["kernel"]["max_ms"]}  ({windows} windows of {calls["loop"]} / {calls["match"]} / {calls["kernel"]} calls)')
    say(f'      query views through the transformer: loop {B * P * M}, match {B * M} (ratio {P});  kernel: {kb["codes_read"]} bytes of codes read, '
        f'{kb["logits_gathered"]} bytes of logits gathered from {kb["view_logits"]} bytes of views, {kb["written"]} bytes written;  '
        f'elements whose bits differ: match vs loop {res["elements_differing_match_vs_loop"]}, kernel vs match '
        f'{res["elements_differing_kernel_vs_match"]} of {B * P * M}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arms', default='mixed')
    ap.add_argument('--windows', type=int, default=WINDOWS)
    ap.add_argument('--shapes', default=None, help='C,B,P,M;... instead of the three shapes')
    ap.add_argument('--out', default=None, help='also write the plain lines to this file')
    args = ap.parse_args()
    shapes = SHAPES if args.shapes is None else [tuple(int(x) for x in s.split(',')) for s in args.shapes.split(';')]
    dev = torch.device('cuda:0')
    out = {}
    for arm in args.arms.split(','):
        for C in sorted({s[0] for s in shapes}):
            vq, tr, _ = build_models(dev, True, arm, 'x3h', sequence_size=C + 1)
            for c, B, P, M in shapes:
                if c == C:
                    out[f'{arm}_C{C}_B{B}_P{P}_M{M}'] = run_shape(dev, arm, vq, tr, C, B, P, M, args.windows)
            del vq, tr
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
