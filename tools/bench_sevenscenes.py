"""time the 7-Scenes pose refinement (viewformer_amd/evaluate_sevenscenes.py) at full size: the models of bench.py's mixed arm with
S = 20 views, a scene bank of N = 7 000 frames, B in {1, 16} queries per call, num_gen_ctx = 9.  In ONE process, alternating, device
events around calls that end in a synchronise, every shape warmed first:
  (a) refinement from the bank (context codes gathered, camera k-NN on the device, only the query frame encoded);
  (b) the same call with reencode=True (the reference's data flow: 20 frames encoded for the first pass, 20 for the second);
  (c) ops.camera_knn alone against compute_camera_distances + torch.topk, N in {1 000, 7 000, 100 000}, Q in {1, 64}, k = 9.
The bank's build (7 000 frames through the encoder once) is timed once and reported separately.  Plain lines, then one JSON line.
No threshold: the numbers are to be read, and (a) slower than (b) at B = 16 would be a defect to explain."""
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_models                                                                     # noqa: E402
from viewformer_amd import ops                                                                      # noqa: E402
from viewformer_amd.evaluate_sevenscenes import (compute_camera_distances, draw_fill_indices,      # noqa: E402
                                                 generate_batch_predictions_using_pose_refinement as refine)
from viewformer_amd.scene_bank import SceneBank                                                     # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

S, N_BANK, NUM_GEN_CTX, DISTINCT = 20, 7000, 9, 500


def timed_ms(fn):
    """one call between device events, ending in a synchronise"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, rounds, warmup=2):
    """{name: [ms per call]} with the candidates taking turns inside every round"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed_ms(fn))
    return out


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), calls=len(ms))


def cameras(n, seed):
    g = np.random.default_rng(seed)
    q = g.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q *= np.where(q[:, :1] >= 0, 1.0, -1.0)
    return np.concatenate((g.normal(0.0, 1.5, size=(n, 3)), q), -1).astype(np.float32)


def main():
    dev = torch.device('cuda:0')
    vq, tr, _ = build_models(dev, True, 'mixed', 'x3h', sequence_size=S)
    out = dict(S=S, bank_frames=N_BANK, num_gen_ctx=NUM_GEN_CTX, models='bench.py mixed arm (fp32-equivalent encoder, bf16 transformer and decoder)')

    # ---- the bank: DISTINCT synthetic frames repeated to N (codes are a function of the frame: the encoder's work is the same), on the device
    frames, _ = synthetic_scene_batch(1, DISTINCT, 128, seed=31)
    bank_frames = torch.from_numpy(frames[0]).to(dev).repeat(N_BANK // DISTINCT, 1, 1, 1)
    bank_cams = cameras(N_BANK, 32)
    SceneBank(vq, bank_frames[:512], bank_cams[:512], batch_size=256)                                            # warm the encoder's shapes
    torch.cuda.synchronize()
    box = {}
    out['bank_build_ms'] = round(timed_ms(lambda: box.update(bank=SceneBank(vq, bank_frames, bank_cams, batch_size=256))), 1)
    bank = box['bank']
    print(f'bank: {N_BANK} frames encoded once in {out["bank_build_ms"]} ms ({out["bank_build_ms"] / N_BANK * 1000:.1f} us per frame)')

    # ---- (a) / (b): refinement from the bank against the re-encoding data flow
    rng = random.Random(5)
    out['refinement'] = {}
    for B, rounds in ((1, 15), (16, 8)):
        qf, qc = synthetic_scene_batch(B, 1, 128, seed=33 + B)
        ctx = [draw_fill_indices(bank, S - 1, rng) for _ in range(B)]
        fill = [draw_fill_indices(bank, S - 1 - NUM_GEN_CTX, rng) for _ in range(B)]
        query = torch.from_numpy(qf).to(dev)                                                       # [B,1,H,W,3]
        ctx_t = torch.tensor(ctx, device=dev)
        images = torch.cat((bank_frames[ctx_t], query), 1)                                         # [B,S,H,W,3]
        cams = torch.cat((bank.cameras[ctx_t], torch.from_numpy(qc).to(dev)), 1)                   # [B,S,7]
        res = {}

        def from_bank():
            res['a'] = refine(bank, tr, vq, query, cams, num_gen_ctx=NUM_GEN_CTX, fill_indices=fill, context_indices=ctx)

        def reencode():
            res['b'] = refine(bank, tr, vq, images, cams, num_gen_ctx=NUM_GEN_CTX, fill_indices=fill, reencode=True)
        t = alternate({'from_bank': from_bank, 'reencode': reencode}, rounds)
        same = all(torch.equal(res['a'][k], res['b'][k]) for k in ('generated_images', 'generated_cameras'))
        r = {k: summary(v) for k, v in t.items()}
        r['identical_predictions'] = bool(same)
        r['ratio_reencode_over_bank'] = round(r['reencode']['median_ms'] / r['from_bank']['median_ms'], 2)
        out['refinement'][f'B{B}'] = r
        print(f'refinement B={B:2d}: (a) from the bank {r["from_bank"]["median_ms"]:9.3f} ms  (b) reencode {r["reencode"]["median_ms"]:9.3f} ms  '
              f'(b)/(a) {r["ratio_reencode_over_bank"]:.2f}  [median of {rounds}, min {r["from_bank"]["min_ms"]} / {r["reencode"]["min_ms"]}]  '
              f'predictions identical: {same}')

    # ---- (c): the k-NN kernel against the torch route (about 45 element-wise launches + topk)
    out['camera_knn'] = {}
    reps = 50
    for N in (1000, 7000, 100000):
        db = torch.from_numpy(cameras(N, 40 + N % 7)).to(dev)
        for Q in (1, 64):
            q = torch.from_numpy(cameras(Q, 50 + Q)).to(dev)
            keep = {}

            def kernel():
                for _ in range(reps):
                    keep['k'] = ops.camera_knn(db, q, NUM_GEN_CTX, 0.3)

            def torch_route():
                for _ in range(reps):
                    keep['t'] = torch.topk(compute_camera_distances(db, q[:, None]), NUM_GEN_CTX, dim=-1, largest=False).indices
            t = alternate({'kernel': kernel, 'torch': torch_route}, 5, warmup=1)
            us = {k: round(statistics.median(v) / reps * 1000, 1) for k, v in t.items()}
            agree = float((keep['k'].long() == keep['t']).all(-1).float().mean())
            out['camera_knn'][f'N{N}_Q{Q}'] = dict(kernel_us=us['kernel'], torch_us=us['torch'], same_index_lists=round(agree, 3))
            print(f'camera_knn N={N:6d} Q={Q:2d} k={NUM_GEN_CTX}: kernel {us["kernel"]:8.1f} us  torch route {us["torch"]:8.1f} us  '
                  f'(median of 5 x {reps} calls; queries with identical index lists: {agree:.3f})')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
