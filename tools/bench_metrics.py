"""time the evaluation metrics at the evaluator's batch (128 pairs of 128 x 128 x 3 uint8 images): vf_image_metrics_u8 alone, and
metrics.Evaluator.update_state without and with LPIPS (VGG-16, random weights of the real shapes) — microseconds per call, one JSON
line.  No threshold: the LPIPS share is to be read against the inference step of the same batch (bench.py's headline)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viewformer_amd import ops                                   # noqa: E402
from viewformer_amd.lpips import LPIPS, make_lpips_weights        # noqa: E402
from viewformer_amd.metrics import Evaluator                     # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch         # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


def main():
    dev = torch.device('cuda:0')
    n, size = 128, 128
    frames, cams = synthetic_scene_batch(n, 2, size, seed=3)
    gt = torch.from_numpy(frames[:, 0]).to(dev)
    gen = torch.from_numpy(frames[:, 1]).to(dev)
    cam_gt = torch.from_numpy(cams[:, 0]).to(dev)
    cam_gen = torch.from_numpy(cams[:, 1]).to(dev)
    batch = dict(ground_truth_cameras=cam_gt, generated_cameras=cam_gen, ground_truth_images=gt, generated_images=gen)
    out = dict(pairs=n, image=[size, size, 3])
    out['kernel_us'] = timed(lambda: ops.image_metrics_u8(gt, gen), 200)
    ev = Evaluator()
    out['update_state_us'] = timed(lambda: ev.update_state(**batch), 100)
    ev_lp = Evaluator(lpips=LPIPS(make_lpips_weights(seed=0), dev))
    out['update_state_lpips_us'] = timed(lambda: ev_lp.update_state(**batch), 10, warmup=2)
    gflop = 2 * 2 * n * sum(cin * cout * 9 * (size >> s) ** 2 for s, layers in enumerate(
        [[(3, 64), (64, 64)], [(64, 128), (128, 128)], [(128, 256), (256, 256), (256, 256)], [(256, 512), (512, 512), (512, 512)],
         [(512, 512), (512, 512), (512, 512)]]) for cin, cout in layers) / 1e9
    out['lpips_vgg_gflop'] = round(gflop, 1)
    out['lpips_tflops'] = round(gflop / out['update_state_lpips_us'] * 1e3, 1)        # GFLOP per us = PFLOP/s
    r = ev_lp.result()
    out['result_sample'] = {k: (v if np.isfinite(v) else str(v)) for k, v in r.items()}
    for k in ('kernel_us', 'update_state_us', 'update_state_lpips_us'):
        out[k] = round(out[k], 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
