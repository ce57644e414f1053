"""time the gradient of a photo's log-likelihood with respect to its camera (viewformer_amd/migt.py: MIGT.score_grad_from_context) against
what the package offered before it: central differences through ``score_from_context``.  Full-size models of bench.py, both arms
('mixed' = the bf16 transformer, 'f32'), (C, B, N) = (6, 1, 1), (6, 1, 128), (6, 16, 8); photos encoded beforehand, poses prepared.
Routes in ONE process, taking turns, every shape warmed first, device events around calls that end in a synchronise, enough calls per
window that a window is not a fraction of a second (5 windows >= 0.4 s); median, min and max of the windows:
  score     one ``score_from_context`` pass (the forward alone)
  grad      one ``score_grad_from_context`` pass (the forward, saving what the backward needs, and the backward)
  fd14      the 14-candidate central-difference gradient: ``score_from_context`` at p +- h e_i, i = 0 ... 6, then 7 differences
  kernel    the n_layer launches of ``ops.attn_prefix_bwd`` alone (csrc/attention_prefix_bwd.hip) on the pass's own operands
Plain lines, then one JSON line; ``--out FILE`` also writes the plain lines there (profiles/refine.txt)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models                                                                     # noqa: E402
from tools.bench_score import LINES, WINDOWS, alternate, say, summary                              # noqa: E402
from viewformer_amd import ops                                                                     # noqa: E402
from viewformer_amd.render import ViewRenderer, query_poses                                        # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                           # noqa: E402

SHAPES = [(6, 1, 1), (6, 1, 128), (6, 16, 8)]
FD_STEP = 1e-3


def run_shape(dev, arm, vq, tr, C, B, N, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    cfg = tr.config
    t, d, H = cfg.token_image_size, cfg.d_model, cfg.n_head
    L = t * t
    r = ViewRenderer(tr, vq).set_context(images=frames[:, :C].contiguous(), cameras=cams[:, :C].contiguous())
    codes = vq.encode(frames[:, C:].reshape(B * N, 128, 128, 3))[-1].to(torch.int32).view(B, N, t, t)
    poses = query_poses(cams[:, C:].contiguous(), r.transform)
    cache = r.cache
    keep = {}

    def score():
        keep['score'] = tr.score_from_context(cache, poses, codes)['log_likelihood']

    def grad():
        keep['grad'] = tr.score_grad_from_context(cache, poses, codes)['grad_cameras']

    eye = torch.eye(7, device=dev) * FD_STEP

    def fd14():
        g = []
        for i in range(7):
            up = tr.score_from_context(cache, poses + eye[i], codes)['log_likelihood']
            dn = tr.score_from_context(cache, poses - eye[i], codes)['log_likelihood']
            g.append((up - dn) / (2 * FD_STEP))
        keep['fd14'] = torch.stack(g, -1)

    # the kernel alone, on one pass's own operands: every layer's saved q / k / v and its cache, one gradient buffer for all layers
    M = B * N * L
    saved = []
    ids32 = torch.full((M,), tr.mask_token, dtype=torch.int32, device=dev)
    tr._query_rows(cache, ids32, tr._pose_embed(poses).contiguous().view(B * N, d), N, save=saved)
    dout = torch.randn((M, d), dtype=torch.float32, device=dev)
    dqkv = torch.empty((M, 3 * d), dtype=torch.float32, device=dev)
    Cc = cache.capacity

    def kernel():
        for i in range(cfg.n_layer):
            qkv, ckv = saved[i][2], cache.kv[i]
            ops.attn_prefix_bwd(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], ckv[:, 2 * d:], ckv[:, :d], dout, dqkv, B, H, Cc, N, L,
                                3 * d, 3 * d, 3 * d, 3 * d, 3 * d, Cc * L * 3 * d, d, 3 * d)

    tms, calls = alternate({'score': score, 'grad': grad, 'fd14': fd14, 'kernel': kernel}, windows)
    res = {k: summary(v, calls[k]) for k, v in tms.items()}
    res['rows'] = M
    res['grad_over_score'] = round(res['grad']['median_ms'] / res['score']['median_ms'], 3)
    res['fd14_over_grad'] = round(res['fd14']['median_ms'] / res['grad']['median_ms'], 3)
    res['kernel_share_of_grad'] = round(res['kernel']['median_ms'] / res['grad']['median_ms'], 3)
    scale = float(keep['grad'].abs().max())
    res['max_grad'] = scale
    res['max_diff_fd14_vs_grad'] = float((keep['fd14'] - keep['grad']).abs().max())
    say(f'{arm:5s} C={C:2d} B={B:2d} N={N:3d}: score {res["score"]["median_ms"]:8.3f} ms  grad {res["grad"]["median_ms"]:8.3f} ms '
        f'(x{res["grad_over_score"]} of score)  fd14 {res["fd14"]["median_ms"]:8.3f} ms (x{res["fd14_over_grad"]} of grad)  '
        f'kernel x{cfg.n_layer} {res["kernel"]["median_ms"]:8.3f} ms ({res["kernel_share_of_grad"]} of grad)')
    say('      spread [min..max] ' + '  '.join(f'{k} {res[k]["min_ms"]}..{res[k]["max_ms"]}' for k in ('score', 'grad', 'fd14', 'kernel'))
        + f'  ({windows} windows of ' + ' / '.join(str(calls[k]) for k in ('score', 'grad', 'fd14', 'kernel')) + ' calls)')
    say(f'      {M} token rows; largest |gradient| {scale:.3g}, largest difference fd14 (h = {FD_STEP}) - grad {res["max_diff_fd14_vs_grad"]:.2e}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arms', default='mixed,f32')
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
