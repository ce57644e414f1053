"""GPU: the evaluation metrics — vf_image_metrics_u8 against the fp64 restatement of the reference's SSIM and exact integer sums, its
determinism and batch independence, and the evaluators of viewformer_amd/metrics.py end to end on the small models of
tests/test_hip_evaluate_loop.py (64 px frames, a 32 px codebook: the generated images go through the bilinear upsample) against an fp64
restatement of the reference's Evaluator (evaluate_transformer.py:22-67, utils/metrics.py, data/_common.py:19-61)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_metrics import ssim_u8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def models(dev):
    from viewformer_amd.config import VQGANConfig, MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, make_vqgan_weights
    vcfg = VQGANConfig(ch=32, ch_mult=[1, 2, 4], num_res_blocks=1, attn_resolutions=[16], image_size=32, z_channels=32, embed_dim=32, n_embed=128)
    mcfg = MIGTConfig(n_embeddings=128, n_head=2, d_model=128, n_layer=2, token_image_size=8, sequence_size=3, pose_multiplier=0.2)
    vq = VQGAN(vcfg, data_format='NHWC').load_state_dict(make_vqgan_weights(vcfg, seed=1, codebook_scale=0.05)).to(dev)
    tr = MIGT(mcfg).load_state_dict(make_migt_weights(mcfg, seed=1, std=0.05)).to(dev)
    return tr, vq


@pytest.fixture(scope='module')
def predictions(dev, models):
    """two batches of 4 scenes of 64 px frames through evaluate.generate_batch_predictions"""
    from viewformer_amd.evaluate import generate_batch_predictions
    from viewformer_amd.weights import synthetic_scene_batch
    tr, vq = models
    out = []
    for seed in (21, 22):
        frames, cams = synthetic_scene_batch(4, 3, 64, seed=seed)
        out.append(generate_batch_predictions(tr, vq, frames, cams))
    torch.cuda.synchronize()
    assert out[0]['ground_truth_images'].shape[1] == 64 and out[0]['generated_images'].shape[1] == 32
    return out


# ------------------------------------------------------------------ fp64 restatement of the reference's Evaluator
def resize_ref(images, image_size, method=None):
    """data/_common.py:19-61 (resize -> resize_th) on a numpy NHWC uint8 batch, in torch on the CPU as the reference runs it"""
    if images.shape[-2] == image_size:
        return images
    th = torch.from_numpy(np.ascontiguousarray(images)).permute(0, 3, 1, 2)
    if th.shape[-2] == image_size:
        return th.permute(0, 2, 3, 1).numpy()
    th = th.to(torch.float32) / 255.
    if method is None:
        method = 'nearest' if image_size > th.shape[-2] else 'bilinear'
    if method == 'nearest':
        th = torch.nn.functional.interpolate(th, (image_size, image_size), mode='nearest')
    else:
        th = torch.nn.functional.interpolate(th, (image_size, image_size), mode='bilinear', align_corners=False)
    th = th.clamp_(0, 1)
    th = (th * 255.).to(torch.uint8)
    return th.permute(0, 2, 3, 1).numpy()


def _qmul(q1, q2):
    """geometry_tf.py:6-13"""
    w1, x1, y1, z1 = np.moveaxis(q1, -1, 0)
    w2, x2, y2, z2 = np.moveaxis(q2, -1, 0)
    x = x1 * w2 + y1 * z2 - z1 * y2 + w1 * x2
    y = -x1 * z2 + y1 * w2 + z1 * x2 + w1 * y2
    z = x1 * y2 - y1 * x2 + z1 * w2 + w1 * z2
    w = -x1 * x2 - y1 * y2 - z1 * z2 + w1 * w2
    return np.stack((w, x, y, z), -1)


def _l2n(q, eps=1e-12):
    return q / np.sqrt(np.maximum((q * q).sum(-1, keepdims=True), eps))


class RefEvaluator:
    """evaluate_transformer.py:22-67 with the metrics of utils/metrics.py restated in fp64 numpy (lpips: oracle/lpips_oracle.py on x/255)"""

    def __init__(self, image_size=None, lpips_sd=None, resize=resize_ref):
        self.image_size, self.sd, self.resize = image_size, lpips_sd, resize
        self.sq_tot = self.ab_tot = self.pix = 0.0
        self.rmse, self.psnr, self.ssim, self.lpips, self.ang, self.dist = [], [], [], [], [], []
        self.last_images = None

    def update_state(self, ground_truth_cameras, generated_cameras, ground_truth_images, generated_images):
        gt = ground_truth_images.cpu().numpy()
        gen = generated_images.cpu().numpy()
        size = self.image_size or max(gt.shape[-2], gen.shape[-2])
        gt = self.resize(gt, size)
        if gen.shape[-2] != size:
            gen = self.resize(gen, size, 'bilinear')
        self.last_images = (gt, gen)
        a, b = gt.astype(np.float64), gen.astype(np.float64)
        d2 = (a - b) ** 2
        self.sq_tot += d2.mean(-1).sum()                                      # MeanSquaredError: channel mean per pixel, mean over pixels
        self.ab_tot += np.abs(a - b).mean(-1).sum()
        self.pix += d2.shape[0] * d2.shape[1] * d2.shape[2]
        m = d2.mean((1, 2, 3))
        self.rmse += list(np.sqrt(m))                                         # ImageRMSE on 0..255
        with np.errstate(divide='ignore'):
            self.psnr += list(-10 * np.log10(m / 255.0 ** 2))                 # tf.image.psnr(max_val=1) on x/255
        self.ssim += list(ssim_u8(gt, gen))
        if self.sd is not None:
            from oracle import lpips_oracle as lo
            x = torch.from_numpy(a / 255).permute(0, 3, 1, 2)
            y = torch.from_numpy(b / 255).permute(0, 3, 1, 2)
            self.lpips += list(lo.distance(self.sd, x, y).numpy())
        if generated_cameras is not None:
            x1 = ground_truth_cameras.cpu().numpy().astype(np.float64)
            x2 = generated_cameras.cpu().numpy().astype(np.float64)
            self.dist += list(np.linalg.norm(x1[..., :3] - x2[..., :3], axis=-1).reshape(-1))
            diff = _qmul(_l2n(x1[..., 3:]), _l2n(x2[..., 3:]) * np.array([1, -1, -1, -1]))
            self.ang += list(2 * np.arcsin(np.linalg.norm(diff[..., 1:], axis=-1)).reshape(-1))

    def result(self):
        def mean(v):
            v = np.asarray(v, np.float64)
            return float(np.where(np.isnan(v), 0, v).sum() / len(v)) if len(v) else 0.0     # AllowNanMean's NaN -> 0, weight 1

        def median(v):
            v = np.sort(np.asarray(v, np.float64))
            if not len(v):
                return 0.0
            return float(v[(len(v) - 1) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))
        r = {'loc-angle': mean(self.ang), 'loc-dist': mean(self.dist), 'loc-angle-med': median(self.ang), 'loc-dist-med': median(self.dist),
             'mse': self.sq_tot / self.pix if self.pix else 0.0, 'rmse': mean(self.rmse), 'mae': self.ab_tot / self.pix if self.pix else 0.0,
             'psnr': mean(self.psnr)}
        if self.sd is not None:
            r['lpips'] = mean(self.lpips)
        r['ssim'] = mean(self.ssim)
        return r


def _close(got, want, rel=1e-6):
    assert list(got) == list(want), (list(got), list(want))
    for k in want:
        if math.isinf(want[k]):
            assert got[k] == want[k], k
        else:
            assert got[k] == pytest.approx(want[k], rel=rel, abs=1e-12), (k, got[k], want[k])


# ------------------------------------------------------------------ the kernel
def _contents(n, H, W, C, rng):
    from viewformer_amd.weights import synthetic_scene_batch
    a = rng.integers(0, 256, size=(n, H, W, C), dtype=np.uint8)
    noise = np.clip(a.astype(np.int32) + rng.integers(-40, 41, size=a.shape), 0, 255).astype(np.uint8)
    cases = {'random': (a, rng.integers(0, 256, size=a.shape, dtype=np.uint8)), 'noisy': (a, noise)}
    if H == W and C == 3:
        f, _ = synthetic_scene_batch(n, 2, H, seed=int(rng.integers(1000)))
        cases['lowpass'] = (f[:, 0], f[:, 1])
    cases['constant'] = (np.full(a.shape, 77, np.uint8), np.full(a.shape, 200, np.uint8))
    cases['0_vs_255'] = (np.zeros(a.shape, np.uint8), np.full(a.shape, 255, np.uint8))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    board = (((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None].repeat(n, 0).repeat(C, 3)
    cases['checkerboard'] = (board, a)
    cases['checkerboard_inverted'] = (board, 255 - board)
    return cases


@pytest.mark.parametrize('n,H,W,C', [(128, 128, 128, 3), (3, 37, 53, 3), (4, 7, 7, 1), (2, 256, 256, 3), (3, 96, 128, 4)])
def test_image_metrics_kernel_matches_the_fp64_restatement(dev, n, H, W, C):
    from viewformer_amd import ops
    rng = np.random.default_rng(H * 1000 + W + C)
    for name, (a, b) in _contents(n, H, W, C, rng).items():
        if n == 128 and name not in ('random', 'lowpass', 'constant'):
            continue                                                    # (the fp64 restatement of 128 pairs per case is the slow part)
        sums, ssim = ops.image_metrics_u8(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
        sums, ssim = sums.cpu().numpy(), ssim.cpu().numpy()
        d = a.astype(np.int64) - b.astype(np.int64)
        assert np.array_equal(sums[:, 0], (d * d).sum((1, 2, 3))), name
        assert np.array_equal(sums[:, 1], np.abs(d).sum((1, 2, 3))), name
        want = ssim_u8(a, b)
        err = np.abs(ssim - want).max()
        assert err < 1e-6, (name, err)
        same_sums, same = ops.image_metrics_u8(torch.from_numpy(a).to(dev), torch.from_numpy(a).to(dev))
        assert torch.all(same == 1.0), (name, same)                     # identical pairs: exactly 1
        assert torch.all(same_sums == 0)


def test_identical_pair_gives_ssim_one_mse_zero_psnr_inf(dev):
    from viewformer_amd.metrics import CodebookEvaluator
    from viewformer_amd.weights import synthetic_scene_batch
    f, _ = synthetic_scene_batch(3, 1, 64, seed=4)
    x = torch.from_numpy(f[:, 0]).to(dev)
    ev = CodebookEvaluator()
    ev.update_state(x, x.clone())
    r = ev.result()
    assert r['ssim'] == 1.0 and r['mse'] == 0.0 and r['mae'] == 0.0 and r['rmse'] == 0.0 and r['psnr'] == math.inf


def test_image_metrics_are_deterministic_and_independent_of_the_batch(dev):
    from viewformer_amd import ops
    rng = np.random.default_rng(11)
    a = torch.from_numpy(rng.integers(0, 256, size=(128, 128, 128, 3), dtype=np.uint8)).to(dev)
    b = torch.from_numpy(np.clip(a.cpu().numpy().astype(np.int32) + rng.integers(-30, 31, size=a.shape), 0, 255).astype(np.uint8)).to(dev)
    s1, q1 = ops.image_metrics_u8(a, b)
    s2, q2 = ops.image_metrics_u8(a, b)
    assert torch.equal(s1, s2) and torch.equal(q1, q2)
    for i in (0, 1, 63, 127):
        si, qi = ops.image_metrics_u8(a[i:i + 1].clone(), b[i:i + 1].clone())
        assert torch.equal(si[0], s1[i]) and torch.equal(qi[0], q1[i]), i
    sh, qh = ops.image_metrics_u8(a[64:], b[64:])
    assert torch.equal(sh, s1[64:]) and torch.equal(qh, q1[64:])


def test_image_metrics_bad_arguments_launch_nothing(dev):
    from viewformer_amd import _lib
    lib = _lib.load()
    a = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=dev)
    sums = torch.full((2, 2), -7, dtype=torch.int64, device=dev)
    ssim = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(int(lib.vf_image_metrics_workspace_bytes(2, 16, 16, 3)), dtype=torch.uint8, device=dev)
    P = ctypes.c_void_p
    p = [P(t.data_ptr()) for t in (a, a, sums, ssim, ws)]
    for args in ((2, 6, 16, 3), (2, 16, 6, 3), (2, 16, 16, 0), (2, 16, 16, 5), (0, 16, 16, 3)):
        assert lib.vf_image_metrics_u8(p[0], p[1], *args, p[2], p[3], p[4], None) == -1, args
    assert lib.vf_image_metrics_u8(p[0], p[1], 2, 16, 16, 3, p[2], p[3], None, None) == -1
    torch.cuda.synchronize()
    assert torch.all(sums == -7) and torch.all(ssim == -7.0) and torch.all(ws == 0)
    assert lib.vf_image_metrics_u8(p[0], p[1], 2, 16, 16, 3, p[2], p[3], p[4], None) == 0
    torch.cuda.synchronize()
    assert torch.all(sums == 0) and torch.all(ssim == 1.0)


# ------------------------------------------------------------------ the evaluators
def lib_resize(dev):
    from viewformer_amd import ops
    return lambda x, size, method=None: ops.resize_u8(torch.from_numpy(np.ascontiguousarray(x)).to(dev), size, method).cpu().numpy()


def test_evaluator_end_to_end_matches_the_reference_restatement(dev, predictions):
    """every key against the fp64 restatement.  ops.resize_u8 reproduces data/_common.py's resize bit for bit where the existing loops use it
    (nearest when enlarging, bilinear when shrinking: tests/golden/resize.npz); its bilinear ENLARGE — the evaluator's upsample of the 32 px
    generated images — rounds a few values one level apart from torch's CPU kernel.  So the exact comparison resizes with the library, and the
    comparison with torch's resize is held to that one-level bound."""
    from viewformer_amd.metrics import Evaluator
    ev, ref, ref_torch = Evaluator(), RefEvaluator(resize=lib_resize(dev)), RefEvaluator()
    for p in predictions:
        ev.update_state(**p)
        ref.update_state(**p)
        ref_torch.update_state(**p)
        assert np.array_equal(ref.last_images[0], ref_torch.last_images[0])          # ground truth at its own size: untouched
        d = ref.last_images[1].astype(np.int32) - ref_torch.last_images[1].astype(np.int32)
        assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 0.05 * d.size, (np.abs(d).max(), np.count_nonzero(d))
    got = ev.result()
    _close(got, ref.result())
    _close(got, ref_torch.result(), rel=2e-3)
    info = ev.get_progress_bar_info()
    assert list(info) == ['img_psnr', 'cam_loc', 'cam_ang'] and info['img_psnr'] == got['psnr']
    # an explicit image_size: both batches resized to 48 (ground truth shrunk bilinearly, generated images enlarged bilinearly)
    ev, ref = Evaluator(image_size=48), RefEvaluator(image_size=48, resize=lib_resize(dev))
    ev.update_state(**predictions[0])
    ref.update_state(**predictions[0])
    _close(ev.result(), ref.result())


def test_codebook_evaluator_on_the_round_trip(dev, models):
    from viewformer_amd.evaluate import codebook_batch_predictions
    from viewformer_amd.metrics import CodebookEvaluator
    from viewformer_amd.weights import synthetic_scene_batch
    _, vq = models
    f, _ = synthetic_scene_batch(6, 1, 32, seed=8)
    p = codebook_batch_predictions(vq, f[:, 0])
    ev, ref = CodebookEvaluator(), RefEvaluator()
    ev.update_state(**p)
    ref.update_state(None, None, p['ground_truth_images'], p['generated_images'])
    want = {k: v for k, v in ref.result().items() if not k.startswith('loc')}
    _close(ev.result(), want)
    assert list(ev.get_progress_bar_info()) == ['img_rgbl1']


def test_lpips_through_the_evaluator_takes_images_on_0_1(dev, predictions):
    """LPIPSMetric feeds x / 255 into a network that expects [-1, 1] (models/utils.py:293-303): reproduced, and measurably not the
    [-1, 1] value"""
    from oracle import lpips_oracle as lo
    from viewformer_amd.lpips import LPIPS, make_lpips_weights
    from viewformer_amd.metrics import Evaluator
    sd = make_lpips_weights(seed=2)
    ev, ref = Evaluator(lpips=LPIPS(sd, dev)), RefEvaluator(lpips_sd=sd, resize=lib_resize(dev))
    p = predictions[0]
    ev.update_state(**p)
    ref.update_state(**p)
    got, want = ev.result(), ref.result()
    assert list(got)[-2:] == ['lpips', 'ssim'] and 'img_lpips' in ev.get_progress_bar_info()
    assert got['lpips'] == pytest.approx(want['lpips'], rel=2e-5)
    _close({k: v for k, v in got.items() if k != 'lpips'}, {k: v for k, v in want.items() if k != 'lpips'})
    gt, gen = ref.last_images
    x = torch.from_numpy(gt.astype(np.float64) / 255 * 2 - 1).permute(0, 3, 1, 2)
    y = torch.from_numpy(gen.astype(np.float64) / 255 * 2 - 1).permute(0, 3, 1, 2)
    other = float(lo.distance(sd, x, y).mean())
    assert abs(other - got['lpips']) > 1e-3 * abs(other), (other, got['lpips'])


def test_localization_keys_with_a_nan_pose(dev, predictions):
    from viewformer_amd.metrics import Evaluator
    p = dict(predictions[0])
    cams = p['generated_cameras'].clone()
    cams[1] = float('nan')
    p['generated_cameras'] = cams
    ev, ref = Evaluator(), RefEvaluator(resize=lib_resize(dev))
    for q in (p, predictions[1]):
        ev.update_state(**q)
        ref.update_state(**q)
    got, want = ev.result(), ref.result()
    _close(got, want)
    assert not math.isnan(got['loc-angle']) and not math.isnan(got['loc-dist'])
    # without cameras the localization means and medians stay 0.0
    ev = Evaluator()
    ev.update_state(**dict(predictions[0], generated_cameras=None))
    assert [ev.result()[k] for k in ('loc-angle', 'loc-dist', 'loc-angle-med', 'loc-dist-med')] == [0.0] * 4


def test_multi_context_evaluator_is_one_evaluator_per_context_size(dev, models):
    from viewformer_amd import evaluate_multictx
    from viewformer_amd.metrics import Evaluator, MultiContextEvaluator
    from viewformer_amd.weights import synthetic_scene_batch
    tr, vq = models
    frames, cams = synthetic_scene_batch(4, 3, 64, seed=31)
    p = evaluate_multictx.generate_batch_predictions(tr, vq, frames, cams)
    mc = MultiContextEvaluator(3)
    mc.update_state(**p)
    r = mc.result()
    assert list(r) == ['ctx01', 'ctx02']
    for nn in (1, 2):
        ev = Evaluator()
        ev.update_state(p['ground_truth_cameras'], p['generated_cameras'][:, nn], p['ground_truth_images'], p['generated_images'][:, nn])
        assert r[f'ctx{nn:02d}'] == ev.result(), nn
    assert mc.get_progress_bar_info() == ev.get_progress_bar_info()


def test_two_shards_merged_give_the_whole_batch_result(dev, predictions):
    from viewformer_amd.metrics import Evaluator, image_values
    whole = Evaluator()
    shards = [Evaluator(), Evaluator()]
    for p in predictions:
        whole.update_state(**p)
        for s, sl in zip(shards, (slice(0, 1), slice(1, None))):
            s.update_state(**{k: v[sl] for k, v in p.items()})
    merged = Evaluator().merge(shards[0].state(), shards[1].state())
    rw, rm = whole.result(), merged.result()
    assert list(rw) == list(rm)
    for k in rw:
        assert rm[k] == pytest.approx(rw[k], rel=1e-12, abs=0), k
    # the per-image values do not depend on the shard
    p = predictions[0]
    vw = image_values(p['ground_truth_images'], p['generated_images'])
    parts = [image_values(p['ground_truth_images'][sl], p['generated_images'][sl]) for sl in (slice(0, 1), slice(1, None))]
    for k in ('sum_sq', 'sum_abs', 'ssim'):
        assert torch.equal(torch.cat([q[k] for q in parts]), vw[k]), k


def test_update_state_does_not_synchronise(dev, predictions):
    if not hasattr(torch.cuda, 'set_sync_debug_mode'):
        pytest.skip('this torch has no sync debug mode')
    from viewformer_amd.metrics import Evaluator, MultiContextEvaluator
    ev = Evaluator()
    ev.update_state(**predictions[0])                                   # first use: library load, allocator warm-up
    p = predictions[1]
    mcp = dict(p, generated_images=torch.stack([p['generated_images']] * 3, 1), generated_cameras=torch.stack([p['generated_cameras']] * 3, 1))
    mc = MultiContextEvaluator(3)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ev.update_state(**p)
        mc.update_state(**mcp)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert ev.result()['mse'] > 0
