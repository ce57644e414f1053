"""Evaluation metrics of the reference's evaluators on MI355X: PSNR, SSIM, MSE / RMSE / MAE, LPIPS and the two pose errors with their
medians — the second step of ``generate_batch_predictions`` -> ``Evaluator.update_state`` -> ``results.json``.

Drop-ins for ``Evaluator`` of viewformer/evaluate/evaluate_transformer.py:22-67 (``Evaluator`` here), ``Evaluator`` of
evaluate_codebook.py:19-49 (``CodebookEvaluator``) and ``MultiContextEvaluator`` of evaluate_transformer_multictx.py:13-35 (also used by
evaluate_transformer_multictx_allimg.py:127,179-183).  Their ``update_state`` takes the dict the matching loop of this package returns
(``evaluate.generate_batch_predictions``, ``evaluate.codebook_batch_predictions``, ``evaluate_multictx.generate_batch_predictions``); for
``evaluate_allimg.evaluate_sequence`` pass the frames of ``eval_frames`` as the reference does (:179-183).

The reference's semantics, restated (these are what the paper's numbers were computed with):

* Resizing (evaluate_transformer.py:36-46): ``image_size=None`` means ``max(gt.shape[-2], gen.shape[-2])``; the ground truth goes through
  ``resize`` with the default method, a generated batch whose ``shape[-2]`` differs through ``resize(..., 'bilinear')`` — both
  ``ops.resize_u8`` (bit-identical to data/_common.py:19-61).
* SSIM (utils/metrics.py:17-69,177-184): 7x7 uniform window, VALID, per channel, sample covariance (49/48),
  ``S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))`` on x/255 with data_range 1 — and **K1 = 1**, not 0.01:
  ``SSIMMetric`` calls ``ssim(gt, gen, 1)`` (:183) and the third positional argument is K1, so C1 = 1 and C2 = 0.03^2.  Per image the mean
  over H', W' and C; the reported value is the mean over images.
* ``mse`` / ``mae`` (Keras ``MeanSquaredError`` / ``MeanAbsoluteError`` on the uint8 images cast to float32, evaluate_transformer.py:30-32):
  on the 0..255 scale, a per-pixel mean over channels, then a mean over **all pixels** of all updates (pixel-weighted).
* ``rmse`` (:164-171): per image ``sqrt(mean((a-b)^2))`` on 0..255, mean over images.
* ``psnr`` (:187-194, ``tf.image.psnr`` with max_val 1): per image ``-10 log10(mse)`` on [0,1], mean over images.  An identical pair gives
  ``+inf`` and then so does the mean, as in the reference; nothing is clamped (the clamp of ``MIGTTrainer.test_step`` is that step's own).
* ``lpips`` (:197-215, models/utils.py:293-303): the images converted to **[0,1]** go into an LPIPS whose ``normalize=False`` expects
  [-1,1]; reproduced by calling ``viewformer_amd.lpips.LPIPS`` on x/255.  The network weights cannot ship with this package, so the
  evaluators take an optional ``LPIPS`` instance: the ``lpips`` key (and ``img_lpips`` of the progress info) is present only when one was
  given.
* ``loc-dist`` = ``||xyz_gt - xyz_gen||``, ``loc-angle`` = ``2 asin(||(q_gt conj(q_gen))[1:]||)`` on l2-normalised quaternions (eps 1e-12)
  (:89-113), both ``AllowNanMean`` (:75-86) — whose NaN handling overwrites ``values`` before taking ``isnan`` (:85-86), so **a NaN counts
  as 0 with weight 1**.  ``loc-*-med`` (:116-161) is the median of every stored value (even count: the mean of the two middle ones;
  nothing stored: 0); NaN values sort last.  The pose errors are evaluated in fp64 (the reference: fp32).
* A mean that was never updated reports 0.0 (Keras ``div_no_nan``): ``loc-*`` when ``generated_cameras`` is None.

Nothing in ``update_state`` synchronises with the host: sums and counts are fp64 device tensors, the median values stay on the device,
one ``vf_image_metrics_u8`` launch pair per update (plus the resizes and LPIPS where they apply).  ``result()`` synchronises once.
``state()`` / ``merge(*states)`` combine evaluators that saw disjoint shards into the single-pass result.

The accumulators (``MetricState``) take per-image values and know nothing of the kernel: they run on CPU tensors too.
"""
import json
import os
from collections import OrderedDict

import torch

from . import geometry
from . import ops

# result key order of the reference (evaluate_transformer.py:25-35: localization metrics first, then the image metrics)
CAMERA_KEYS = ('loc-angle', 'loc-dist', 'loc-angle-med', 'loc-dist-med')
IMAGE_KEYS = ('mse', 'rmse', 'mae', 'psnr', 'lpips', 'ssim')
_PIXEL_WEIGHTED = ('mse', 'mae')
# the evaluators' outputs that update_state accepts and ignores (return_codes=True extras, the multi-context / codebook loops' codes)
_PREDICTION_EXTRAS = frozenset(('codes', 'generated_codes', 'logits_last', 'decoded', 'pose_last', 'eval_frames'))


class MetricState:
    """Sums and counts of the means (fp64, one [K, 2] tensor on the device of the first update) and the stored values of the medians.

    ``images``: the image metrics (``lpips``: with the LPIPS mean); ``cameras``: the pose errors.  Per-image values go in, ``result()``
    gives the ordered dict of Python floats."""

    def __init__(self, images: bool = True, lpips: bool = False, cameras: bool = True):
        self.lpips = bool(lpips) and images
        keys = []
        if cameras:
            keys += list(CAMERA_KEYS)
        if images:
            keys += [k for k in IMAGE_KEYS if k != 'lpips' or self.lpips]
        self.keys = tuple(keys)
        # the accumulator's rows: pixel-weighted means first (their counts advance together), then the per-image means, then the poses
        self.mean_keys = tuple([k for k in _PIXEL_WEIGHTED if k in keys] + [k for k in IMAGE_KEYS if k in keys and k not in _PIXEL_WEIGHTED]
                               + [k for k in CAMERA_KEYS[:2] if k in keys])
        self.median_keys = tuple(k for k in CAMERA_KEYS[2:] if k in keys)
        self._row = {k: i for i, k in enumerate(self.mean_keys)}
        self._acc = None
        self._med = {k: [] for k in self.median_keys}
        self._med_len = {k: 0 for k in self.median_keys}

    def _accumulator(self, device):
        if self._acc is None:
            self._acc = torch.zeros((len(self.mean_keys), 2), dtype=torch.float64, device=device)
        return self._acc

    def update_images(self, sum_sq, sum_abs, ssim, pixels, channels, lpips=None):
        """per-image values of one update, [n] tensors: ``sum_sq`` / ``sum_abs`` the sums of (a-b)^2 / |a-b| on 0..255 over the image,
        ``ssim`` its mean SSIM, ``lpips`` its distance (required exactly when the state has the LPIPS mean); ``pixels`` = H*W and
        ``channels`` = C of the images (host ints)"""
        if (lpips is None) == self.lpips:
            raise ValueError('lpips values are required exactly when the evaluator was given an LPIPS network')
        n = int(sum_sq.shape[0])
        if n == 0:
            return
        sq = sum_sq.to(torch.float64)
        ab = sum_abs.to(torch.float64)
        hwc = float(pixels * channels)
        per = {'mse': sq / channels, 'mae': ab / channels,                       # per-pixel channel means, summed over the pixels
               'rmse': torch.sqrt(sq / hwc),
               'psnr': -10.0 * torch.log10(sq / (hwc * 255.0 * 255.0)),          # mse on [0,1]; 0 -> +inf
               'ssim': ssim.to(torch.float64)}
        if self.lpips:
            per['lpips'] = lpips.to(torch.float64)
        rows = [k for k in self.mean_keys if k in per]
        i0 = self._row[rows[0]]
        acc = self._accumulator(sq.device)
        acc[i0:i0 + len(rows), 0] += torch.stack([per[k].sum() for k in rows])
        npix = sum(1 for k in rows if k in _PIXEL_WEIGHTED)
        acc[i0:i0 + npix, 1] += float(n * pixels)
        acc[i0 + npix:i0 + len(rows), 1] += float(n)

    def update_cameras(self, angle, dist):
        """per-view pose errors (any shape): the means take NaN as 0 with weight 1 (AllowNanMean, metrics.py:85-86), the medians keep
        the values as they are"""
        angle = angle.reshape(-1).to(torch.float64)
        dist = dist.reshape(-1).to(torch.float64)
        n = int(angle.shape[0])
        if n == 0:
            return
        i0 = self._row['loc-angle']
        acc = self._accumulator(angle.device)
        v = torch.stack([angle, dist])
        acc[i0:i0 + 2, 0] += torch.where(torch.isnan(v), torch.zeros_like(v), v).sum(1)
        acc[i0:i0 + 2, 1] += float(n)
        for k, x in (('loc-angle-med', angle), ('loc-dist-med', dist)):
            self._med[k].append(x)
            self._med_len[k] += n

    # ------------------------------------------------------------------ data-parallel merge
    def state(self):
        """plain tensors: ``sums`` / ``counts`` [K] in the order of ``mean_keys``, and the stored values of each median"""
        acc = self._acc if self._acc is not None else torch.zeros((len(self.mean_keys), 2), dtype=torch.float64)
        st = {'sums': acc[:, 0].clone(), 'counts': acc[:, 1].clone()}
        for k in self.median_keys:
            st[k] = torch.cat(self._med[k]) if self._med[k] else torch.zeros(0, dtype=torch.float64, device=acc.device)
        return st

    def merge(self, *states):
        """add the sums / counts and the median values of other evaluators' ``state()`` (same configuration) to this one"""
        for st in states:
            if st['sums'].shape[0] != len(self.mean_keys) or any(k not in st for k in self.median_keys):
                raise ValueError('merge: the state comes from an evaluator of another configuration')
            acc = self._accumulator(st['sums'].device)
            acc[:, 0] += st['sums'].to(acc.device, torch.float64)
            acc[:, 1] += st['counts'].to(acc.device, torch.float64)
            for k in self.median_keys:
                v = st[k].reshape(-1).to(acc.device, torch.float64)
                if v.shape[0]:
                    self._med[k].append(v)
                    self._med_len[k] += int(v.shape[0])
        return self

    def result(self):
        """OrderedDict of Python floats in the reference's key order (one host synchronisation)"""
        parts = []
        if self._acc is not None:
            parts.append(self._acc.reshape(-1))
        for k in self.median_keys:                                  # Median.result (metrics.py:146-155), lengths known on the host
            m = self._med_len[k]
            if m:
                vals = torch.sort(torch.cat(self._med[k])).values
                parts.append(vals[(m - 1) // 2:(m - 1) // 2 + 1] if m % 2 == 1 else 0.5 * (vals[m // 2 - 1:m // 2] + vals[m // 2:m // 2 + 1]))
        host = torch.cat([p.to(parts[0].device) for p in parts]).cpu().tolist() if parts else []
        out, pos = {}, 0
        if self._acc is not None:
            for k in self.mean_keys:
                s, c = host[2 * pos], host[2 * pos + 1]
                out[k] = s / c if c != 0 else 0.0                   # div_no_nan
                pos += 1
            pos *= 2
        else:
            out.update({k: 0.0 for k in self.mean_keys})
        for k in self.median_keys:
            if self._med_len[k]:
                out[k] = float(host[pos])
                pos += 1
            else:
                out[k] = 0.0
        return OrderedDict((k, float(out[k])) for k in self.keys)


# ------------------------------------------------------------------ per-batch values on the GPU
def _device(*tensors, lpips=None):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    if lpips is not None:
        return lpips.dev
    return torch.device('cuda', torch.cuda.current_device())


def image_values(ground_truth_images, generated_images, image_size=None, lpips=None):
    """evaluate_transformer.py:36-46 up to the metrics' inputs: resize both batches as the reference does, then ONE vf_image_metrics_u8
    launch pair (+ LPIPS on x/255).  uint8 [..., H, W, C] -> dict of per-image [n] device tensors for ``MetricState.update_images``."""
    dev = _device(ground_truth_images, generated_images, lpips=lpips)
    gt = torch.as_tensor(ground_truth_images).to(dev, non_blocking=True)
    gen = torch.as_tensor(generated_images).to(dev, non_blocking=True)
    gt = gt.reshape(-1, *gt.shape[-3:])
    gen = gen.reshape(-1, *gen.shape[-3:])
    if image_size is None:
        image_size = max(gt.shape[-2], gen.shape[-2])
    gt = ops.resize_u8(gt, image_size)
    if gen.shape[-2] != image_size:                                  # "when upsampling generated image, we will use bilinear as well"
        gen = ops.resize_u8(gen, image_size, 'bilinear')
    sums, ssim = ops.image_metrics_u8(gt, gen)
    n, H, W, C = gt.shape
    out = dict(sum_sq=sums[:, 0], sum_abs=sums[:, 1], ssim=ssim, pixels=H * W, channels=C, lpips=None)
    if lpips is not None and n:
        # tf.image.convert_image_dtype(uint8 -> float32) = x * float32(1/255): [0,1] into a network that expects [-1,1] (the reference's quirk)
        out['lpips'] = lpips(gt.to(torch.float32).mul_(1.0 / 255.0), gen.to(torch.float32).mul_(1.0 / 255.0))
    elif lpips is not None:
        out['lpips'] = torch.zeros(0, dtype=torch.float32, device=dev)
    return out


def camera_errors(ground_truth_cameras, generated_cameras):
    """CameraOrientationError / CameraPositionError (metrics.py:89-113) per view, in fp64: -> (angle, dist) of shape [...]"""
    x1 = torch.as_tensor(ground_truth_cameras).to(torch.float64)
    x2 = torch.as_tensor(generated_cameras).to(x1.device, torch.float64)
    dist = torch.linalg.vector_norm(x1[..., :3] - x2[..., :3], dim=-1)
    q1 = geometry.quaternion_normalize(x1[..., 3:])
    q2 = geometry.quaternion_normalize(x2[..., 3:])
    diff = geometry.quaternion_multiply(q1, geometry.quaternion_conjugate(q2))
    angle = 2 * torch.asin(torch.linalg.vector_norm(diff[..., 1:], dim=-1))
    return angle, dist


def _check_extras(extras):
    bad = set(extras) - _PREDICTION_EXTRAS
    if bad:
        raise TypeError(f'update_state: unexpected keys {sorted(bad)}')


class _ImageEvaluator:
    def __init__(self, image_size, lpips, cameras):
        self.image_size = image_size
        self.lpips = lpips
        self._state = MetricState(images=True, lpips=lpips is not None, cameras=cameras)

    def update_with_image(self, ground_truth_images, generated_images):
        v = image_values(ground_truth_images, generated_images, self.image_size, self.lpips)
        self._state.update_images(**v)

    def result(self):
        return self._state.result()

    def state(self):
        return self._state.state()

    def merge(self, *states):
        self._state.merge(*states)
        return self


class Evaluator(_ImageEvaluator):
    """evaluate_transformer.py:22-67.  ``lpips``: a ``viewformer_amd.lpips.LPIPS`` (the ``lpips`` key is reported only with one)."""

    def __init__(self, image_size: int = None, lpips=None):
        super().__init__(image_size, lpips, cameras=True)

    def update_with_camera(self, ground_truth_cameras, generated_cameras):
        self._state.update_cameras(*camera_errors(ground_truth_cameras, generated_cameras))

    def update_state(self, ground_truth_cameras, generated_cameras, ground_truth_images, generated_images, **extras):
        _check_extras(extras)
        self.update_with_image(ground_truth_images, generated_images)
        if generated_cameras is not None:
            self.update_with_camera(ground_truth_cameras, generated_cameras)

    def get_progress_bar_info(self):
        r = self.result()
        info = [('img_psnr', r['psnr'])] + ([('img_lpips', r['lpips'])] if 'lpips' in r else [])
        return OrderedDict(info + [('cam_loc', r['loc-dist']), ('cam_ang', r['loc-angle'])])


class CodebookEvaluator(_ImageEvaluator):
    """evaluate_codebook.py:19-49 (keys mse, rmse, mae, psnr, [lpips], ssim)"""

    def __init__(self, image_size: int = None, lpips=None):
        super().__init__(image_size, lpips, cameras=False)

    def update_state(self, ground_truth_images, generated_images, **extras):
        _check_extras(extras)
        self.update_with_image(ground_truth_images, generated_images)

    def get_progress_bar_info(self):
        r = self.result()
        return OrderedDict([('img_rgbl1', r['mae'])] + ([('img_lpips', r['lpips'])] if 'lpips' in r else []))


class MultiContextEvaluator:
    """evaluate_transformer_multictx.py:13-35: one ``Evaluator`` per context size 1 .. S-1, reported as ``ctx01`` ... ``ctx{S-1}``;
    position 0 of ``generated_images`` [B,S,...] / ``generated_cameras`` [B,S,7] (no context) is skipped."""

    def __init__(self, sequence_size: int, image_size: int = None, lpips=None):
        self.sequence_size = sequence_size
        self._evaluators = [Evaluator(image_size=image_size, lpips=lpips) for _ in range(sequence_size - 1)]

    def update_state(self, ground_truth_cameras, generated_cameras, ground_truth_images, generated_images, **extras):
        _check_extras(extras)
        for i in range(1, generated_images.shape[1]):
            gen_cam = generated_cameras[:, i] if generated_cameras is not None else None
            self._evaluators[i - 1].update_state(ground_truth_cameras, gen_cam, ground_truth_images, generated_images[:, i])

    def get_progress_bar_info(self):
        return self._evaluators[-1].get_progress_bar_info()

    def result(self):
        return OrderedDict((f'ctx{i + 1:02d}', e.result()) for i, e in enumerate(self._evaluators))

    def state(self):
        return [e.state() for e in self._evaluators]

    def merge(self, *states):
        for st in states:
            if len(st) != len(self._evaluators):
                raise ValueError('merge: the state comes from a MultiContextEvaluator of another sequence size')
            for e, s in zip(self._evaluators, st):
                e.merge(s)
        return self


def write_results(job_dir, result):
    """``results.json`` as the evaluators write it (evaluate_transformer.py:230-232): ``json.dump(result, f, indent=4)`` (inf -> Infinity)"""
    os.makedirs(job_dir, exist_ok=True)
    path = os.path.join(job_dir, 'results.json')
    with open(path, 'w+') as f:
        json.dump(result, f, indent=4)
    return path
