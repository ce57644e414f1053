"""CPU: the evaluation metrics (viewformer_amd/metrics.py, csrc/image_metrics.hip) without a GPU — the fp64 restatement of the reference's
SSIM (viewformer/utils/metrics.py:17-69) checked against an independent form, the C-ABI's host-side argument rules, and the host
accumulators fed per-image values directly (the reference's weighting, NaN, median and empty-metric semantics, key order, merge,
results.json).  The GPU side is tests/test_hip_metrics.py, which imports the restatement from here."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

from viewformer_amd.metrics import (CAMERA_KEYS, CodebookEvaluator, Evaluator, MetricState, MultiContextEvaluator,
                                    write_results)

TRANSFORMER_KEYS = ['loc-angle', 'loc-dist', 'loc-angle-med', 'loc-dist-med', 'mse', 'rmse', 'mae', 'psnr', 'lpips', 'ssim']
CODEBOOK_KEYS = ['mse', 'rmse', 'mae', 'psnr', 'lpips', 'ssim']


# ------------------------------------------------------------------ fp64 restatement of the reference
def ssim_literal(X, Y, K1=1.0, K2=0.03, win_size=7, data_range=1.0):
    """metrics.py:17-69 line by line in fp64 numpy: X, Y [..., H, W, C] on [0,1] -> [...] (mean over H', W', C).  SSIMMetric passes
    K1 = 1 (metrics.py:183); the signature default 0.01 is NOT what the evaluators use."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    H, W = X.shape[-3], X.shape[-2]
    Ho, Wo = H - win_size + 1, W - win_size + 1

    def filter_func(Z):                       # depthwise_conv2d, kernel filled with 1 / win_size^2, VALID
        out = np.zeros(Z.shape[:-3] + (Ho, Wo, Z.shape[-1]))
        for dy in range(win_size):
            for dx in range(win_size):
                out += Z[..., dy:dy + Ho, dx:dx + Wo, :] * (1 / win_size ** 2)
        return out
    NP = win_size ** 2
    cov_norm = NP / (NP - 1)
    ux, uy = filter_func(X), filter_func(Y)
    uxx, uyy, uxy = filter_func(X * X), filter_func(Y * Y), filter_func(X * Y)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = data_range
    C1 = (K1 * R) ** 2
    C2 = (K2 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    return S.mean(axis=(-3, -2, -1))


def ssim_u8(a, b):
    """the evaluators' SSIM of uint8 [..., H, W, C] images (convert_image_dtype -> x / 255)"""
    return ssim_literal(np.asarray(a, np.float64) / 255.0, np.asarray(b, np.float64) / 255.0)


def _ssim_uniform_filter(X, Y, K1=1.0, K2=0.03):
    """the same quantity through scipy.ndimage.uniform_filter (centred 7-tap means), cropped to the VALID region"""
    from scipy.ndimage import uniform_filter
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    size = (1,) * (X.ndim - 3) + (7, 7, 1)

    def f(Z):
        return uniform_filter(Z, size=size, mode='reflect')[..., 3:-3, 3:-3, :]
    ux, uy = f(X), f(Y)
    vx = (f(X * X) - ux * ux) * 49 / 48
    vy = (f(Y * Y) - uy * uy) * 49 / 48
    vxy = (f(X * Y) - ux * uy) * 49 / 48
    c1, c2 = K1 ** 2, K2 ** 2
    s = (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s.mean(axis=(-3, -2, -1))


def test_ssim_restatement_agrees_with_an_independent_form_and_uses_k1_equal_1():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(3, 37, 53, 3)).astype(np.float64) / 255
    b = np.clip(a + rng.normal(0, 0.1, size=a.shape), 0, 1)
    lit = ssim_literal(a, b)
    ind = _ssim_uniform_filter(a, b)
    assert lit.shape == (3,)
    assert np.max(np.abs(lit - ind)) < 1e-12, (lit, ind)
    # K1 = 1, as SSIMMetric passes it, is a different metric from the textbook K1 = 0.01
    k001 = ssim_literal(a, b, K1=0.01)
    assert np.max(np.abs(k001 - _ssim_uniform_filter(a, b, K1=0.01))) < 1e-12
    assert np.all(np.abs(lit - k001) > 1e-4), (lit, k001)
    dark = a * 0.05                                                      # where the luminance term matters, by far
    assert np.all(ssim_literal(dark, a) > 5 * ssim_literal(dark, a, K1=0.01))
    # identical images: 1; constant images of different levels: the luminance term alone
    assert np.allclose(ssim_literal(a, a), 1.0, rtol=0, atol=1e-15)
    z, o = np.zeros((1, 7, 7, 1)), np.ones((1, 7, 7, 1))
    assert abs(ssim_literal(z, o)[0] - 1.0 / 2.0) < 1e-12               # (0 + 1) / (0 + 1 + 1), the contrast term is C2 / C2


# ------------------------------------------------------------------ C-ABI, host side
@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()
    return _lib.load()


def test_image_metrics_symbols_are_exported_and_the_workspace_query_is_host_only(lib):
    from viewformer_amd import _lib
    for name in ('vf_image_metrics_u8', 'vf_image_metrics_workspace_bytes'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    ws = lib.vf_image_metrics_workspace_bytes
    one = ws(1, 128, 128, 3)
    assert one > 0 and one % 8 == 0
    assert ws(128, 128, 128, 3) == 128 * one                             # per-image partials: linear in the batch
    assert ws(1, 7, 7, 1) > 0 and ws(1, 256, 256, 3) > one
    for bad in ((0, 8, 8, 3), (1, 6, 8, 3), (1, 8, 6, 3), (1, 8, 8, 0), (1, 8, 8, 5)):
        assert ws(*bad) == 0, bad
    assert lib.vf_abi_version() == 20                                    # no existing signature changed


def test_image_metrics_bad_arguments_are_refused_before_any_launch(lib):
    P = ctypes.c_void_p
    d = P(4096)                        # never dereferenced: every case below fails validation on the host
    f = lib.vf_image_metrics_u8
    assert f(None, d, 1, 8, 8, 3, d, d, d, None) == -1
    assert f(d, None, 1, 8, 8, 3, d, d, d, None) == -1
    assert f(d, d, 1, 8, 8, 3, None, d, d, None) == -1
    assert f(d, d, 1, 8, 8, 3, d, None, d, None) == -1
    assert f(d, d, 1, 8, 8, 3, d, d, None, None) == -1
    assert f(d, d, 1, 6, 8, 3, d, d, d, None) == -1                     # H < 7
    assert f(d, d, 1, 8, 6, 3, d, d, d, None) == -1                     # W < 7
    assert f(d, d, 1, 8, 8, 0, d, d, d, None) == -1                     # C < 1
    assert f(d, d, 1, 8, 8, 5, d, d, d, None) == -1                     # C > 4
    assert f(d, d, 0, 8, 8, 3, d, d, d, None) == -1                     # n_img < 1
    assert f(d, d, -3, 8, 8, 3, d, d, d, None) == -1


def test_image_metrics_wrapper_refuses_cpu_tensors(lib):
    from viewformer_amd import ops, _lib
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_lib.VfError):
        ops.image_metrics_u8(x, x)


# ------------------------------------------------------------------ accumulators
def _t(x):
    return torch.tensor(x, dtype=torch.float64)


def test_mse_and_mae_are_pixel_weighted_the_rest_image_weighted():
    st = MetricState(cameras=False)
    # update 1: two 2x2x3 images; update 2: one 4x4x3 image (4x the pixels)
    st.update_images(_t([12.0, 0.0]), _t([6.0, 0.0]), _t([0.5, 1.0]), pixels=4, channels=3)
    st.update_images(_t([480.0]), _t([96.0]), _t([0.2]), pixels=16, channels=3)
    r = st.result()
    assert list(r) == ['mse', 'rmse', 'mae', 'psnr', 'ssim']
    # mse: per-pixel channel means summed over all 8 + 16 pixels
    assert r['mse'] == pytest.approx((12 / 3 + 0 + 480 / 3) / 24, rel=1e-15)
    assert r['mae'] == pytest.approx((6 / 3 + 96 / 3) / 24, rel=1e-15)
    # rmse / psnr / ssim: a mean over the three images
    per_mse = [12 / 12, 0.0, 480 / 48]
    assert r['rmse'] == pytest.approx(sum(math.sqrt(m) for m in per_mse) / 3, rel=1e-15)
    assert r['ssim'] == pytest.approx((0.5 + 1.0 + 0.2) / 3, rel=1e-15)
    assert r['psnr'] == math.inf                                        # the identical pair: +inf, not clamped
    st2 = MetricState(cameras=False)
    st2.update_images(_t([12.0, 480.0]), _t([6.0, 0.0]), _t([0.5, 1.0]), pixels=4, channels=3)
    want = sum(-10 * math.log10(s / 12 / 255 ** 2) for s in (12.0, 480.0)) / 2
    assert st2.result()['psnr'] == pytest.approx(want, rel=1e-14)


def test_nan_pose_error_counts_as_zero_with_weight_one_and_medians():
    st = MetricState(images=False)
    st.update_cameras(_t([0.1, float('nan'), 0.5]), _t([1.0, 2.0, 4.0]))
    r = st.result()
    assert list(r) == list(CAMERA_KEYS)
    assert r['loc-angle'] == pytest.approx(0.6 / 3, rel=1e-15)          # NaN -> 0, still counted (metrics.py:85-86)
    assert r['loc-dist'] == pytest.approx(7.0 / 3, rel=1e-15)
    assert r['loc-dist-med'] == 2.0                                     # odd count: the middle value
    assert r['loc-angle-med'] == 0.5                                    # NaN sorts last
    st.update_cameras(_t([0.2]), _t([10.0]))
    r = st.result()
    assert r['loc-dist-med'] == 3.0                                     # even count: mean of 2 and 4
    assert r['loc-angle-med'] == pytest.approx(0.35, rel=1e-15)


def test_metrics_never_updated_report_zero_and_key_order():
    r = MetricState(lpips=True).result()
    assert list(r) == TRANSFORMER_KEYS and all(v == 0.0 for v in r.values())
    # camera means and medians when generated_cameras was always None: 0.0 (div_no_nan / Median's default)
    st = MetricState()
    st.update_images(_t([3.0]), _t([3.0]), _t([0.9]), pixels=1, channels=3)
    r = st.result()
    assert [r[k] for k in CAMERA_KEYS] == [0.0] * 4 and r['mse'] == 1.0
    assert list(Evaluator().result()) == [k for k in TRANSFORMER_KEYS if k != 'lpips']
    assert list(CodebookEvaluator().result()) == [k for k in CODEBOOK_KEYS if k != 'lpips']
    mc = MultiContextEvaluator(4).result()
    assert list(mc) == ['ctx01', 'ctx02', 'ctx03']
    assert all(list(v) == [k for k in TRANSFORMER_KEYS if k != 'lpips'] for v in mc.values())
    with pytest.raises(ValueError):                                     # lpips values iff the evaluator has a network
        MetricState().update_images(_t([1.0]), _t([1.0]), _t([1.0]), pixels=1, channels=3, lpips=_t([0.1]))
    with pytest.raises(ValueError):
        MetricState(lpips=True).update_images(_t([1.0]), _t([1.0]), _t([1.0]), pixels=1, channels=3)


def _feed(st, rng, n, lo, hi):
    for i in range(lo, hi):
        sq = _t(rng.integers(1, 10 ** 6, size=n).astype(np.float64))
        st.update_images(sq, sq / 7, _t(rng.uniform(0, 1, size=n)), pixels=64, channels=3, lpips=_t(rng.uniform(0, 1, size=n)))
        ang = rng.uniform(0, 3, size=n)
        if i == 1:
            ang[0] = np.nan
        st.update_cameras(_t(ang), _t(rng.uniform(0, 5, size=n)))


def test_merge_of_two_halves_equals_one_pass():
    whole = MetricState(lpips=True)
    _feed(whole, np.random.default_rng(5), 4, 0, 6)
    a, b = MetricState(lpips=True), MetricState(lpips=True)
    rng = np.random.default_rng(5)
    _feed(a, rng, 4, 0, 3)
    _feed(b, rng, 4, 3, 6)
    merged = MetricState(lpips=True).merge(a.state(), b.state())
    rw, rm = whole.result(), merged.result()
    assert list(rw) == list(rm) == TRANSFORMER_KEYS
    for k in rw:
        assert rm[k] == pytest.approx(rw[k], rel=1e-12, abs=0), k
    assert rm['loc-angle-med'] == rw['loc-angle-med'] and rm['loc-dist-med'] == rw['loc-dist-med']
    # merging into a shard that already holds values; the state is plain tensors
    st = a.state()
    assert set(st) == {'sums', 'counts', 'loc-angle-med', 'loc-dist-med'} and all(torch.is_tensor(v) for v in st.values())
    again = a.merge(b.state()).result()
    for k in rw:
        assert again[k] == pytest.approx(rw[k], rel=1e-12, abs=0), k
    with pytest.raises(ValueError):
        MetricState(lpips=False).merge(b.state())


def test_write_results_round_trips_and_writes_infinity(tmp_path):
    st = MetricState(cameras=False)
    st.update_images(_t([0.0]), _t([0.0]), _t([1.0]), pixels=4, channels=3)
    r = st.result()
    path = write_results(str(tmp_path / 'job'), r)
    text = open(path).read()
    assert '"psnr": Infinity' in text and text.startswith('{\n    "mse"')
    back = json.loads(text)
    assert list(back) == list(r) and back == dict(r)
