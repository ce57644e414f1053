"""Codebook (VQGAN) training step on the GPU vs the oracle restatement and the reference-recorded golden.

The oracle (oracle/vqgan_train_oracle.py, fp64 autograd) is pinned to the reference by tests/test_oracle_vqgan.py; here the HIP
training step (viewformer_amd/vqgan_train.py) is compared with both."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'vqgan_train_tiny.npz')


def _summary(t):
    f = np.asarray(t, dtype=np.float64).reshape(-1)
    n = f.size
    return np.array([np.linalg.norm(f), f.sum(), f[0], f[n // 2], f[n - 1]])


def _tiny():
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.weights import make_vqgan_weights
    g = np.load(GOLD)
    cfg = VQGANConfig(ch=32, ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[16], image_size=32, z_channels=32, embed_dim=32,
                      n_embed=64, perceptual_weight=0.0, codebook_weight=1.0, learning_rate=1e-3)
    sd = make_vqgan_weights(cfg, seed=int(g['seed']), codebook_scale=float(g['codebook_scale']))
    return g, cfg, sd


def _trainer(cfg, sd, **kw):
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.vqgan_train import VQGANTrainer
    model = VQGAN(cfg, device='cuda')
    model.load_state_dict(sd)
    return VQGANTrainer(model, **kw)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def test_training_step_matches_reference_golden_and_oracle():
    """loss terms, all 154 gradients, the EMA codebook after the forward, and two Adam steps"""
    from oracle import vqgan_oracle as vq
    from oracle import vqgan_train_oracle as vt
    g, cfg, sd = _tiny()
    x = vq.preprocess_u8(torch.from_numpy(g['frames']))                      # NCHW float32 in [-1, 1]
    names = [str(n) for n in g['param_names']]
    tr = _trainer(cfg, sd)
    assert sorted(tr.names) == sorted(names)
    m = tr.train_step(x, apply_update=False)
    torch.cuda.synchronize()
    assert abs(float(m['total_loss']) - float(g['loss'])) < 5e-6
    assert abs(float(m['rec_loss']) - float(g['rec_loss'])) < 5e-6
    assert abs(float(m['quant_loss']) - float(g['quant_loss'])) < 2e-6
    # ---- every gradient against the fp64 oracle (elementwise) and the reference's recorded summaries
    grads, metrics, extra = vt.gradients({k: np.asarray(v) for k, v in sd.items()}, cfg, x)
    assert torch.equal(tr.last_indices.cpu().view(-1), extra['ind'].view(-1))
    worst, bad = 0.0, []
    for i, n in enumerate(names):
        got = tr.g(n).cpu().numpy()
        want = grads[n].numpy()
        gn = float(g['grad_summary'][i][0])
        if gn < 1e-6:                                                         # mathematically zero (bias before a per-channel norm)
            if not np.abs(got).max() < 1e-6:
                bad.append((n, 'nonzero', float(np.abs(got).max())))
            continue
        r = _rel(got, want)
        worst = max(worst, r)
        s = _summary(got)
        if not (r < 2e-4 and np.allclose(s[[0, 2, 3, 4]], g['grad_summary'][i][[0, 2, 3, 4]], rtol=2e-3, atol=1e-6)):
            bad.append((n, r, float(np.linalg.norm(got)), float(np.linalg.norm(want))))
    assert not bad, '\n'.join(map(str, bad))
    for key in g.files:
        if key.startswith('grad:'):
            assert np.allclose(tr.g(key[5:]).cpu().numpy(), g[key], rtol=2e-3, atol=1e-6), key
    print('worst relative gradient error vs fp64 oracle', worst)
    # ---- the forward moved the codebook
    qs = tr.quantizer.state_dict()
    assert np.allclose(qs['quantize.embeddings'].cpu().numpy(), g['E_after_fwd'], rtol=1e-4, atol=1e-6)
    assert np.allclose(qs['quantize.ema_cluster_size_hidden'].cpu().numpy(), g['cs_after_fwd'], rtol=1e-5, atol=1e-7)
    # ---- two optimizer steps
    tr.apply_gradients()
    lr = float(g['lr'])
    for step in (1, 2):
        if step == 2:
            m2 = tr.train_step(x)
            assert abs(float(m2['total_loss']) - float(g['loss_step2'])) < 1e-4                # the loss of the second forward
        want = g[f'param_summary_step{step}']
        for i, n in enumerate(names):
            p = tr.p(n).cpu().numpy().astype(np.float64)
            if g['grad_summary'][i][0] < 1e-6:
                assert np.all(np.abs(p - np.asarray(sd[n], np.float64)) <= 1.01 * lr * step), (step, n)
                continue
            got = _summary(p)
            assert np.allclose(got[[0, 2, 3, 4]], want[i][[0, 2, 3, 4]], rtol=1e-4, atol=2.1 * lr * step), (step, n)
            assert abs(got[0] - want[i][0]) < 1e-4 * want[i][0] + 1e-6, (step, n)


def test_training_reduces_the_loss_and_syncs_back():
    """a few steps on one batch drive the reconstruction loss down; sync_model() makes the inference model use the trained weights"""
    from oracle import vqgan_oracle as vq
    g, cfg, sd = _tiny()
    x = vq.preprocess_u8(torch.from_numpy(g['frames']))
    tr = _trainer(cfg, sd)
    first = float(tr.train_step(x)['total_loss'])
    for _ in range(15):
        last = float(tr.train_step(x)['total_loss'])
    assert np.isfinite(last) and last < 0.8 * first, (first, last)
    model = tr.sync_model()
    codes = model.encode_codes(x.cuda())
    assert codes.shape == (x.shape[0], 16, 16)


def test_global_norm_clip_scales_the_flat_gradient():
    """gradient_clip_val at half the fp64 norm of the unclipped gradient: after apply_gradients() flat_g is the unclipped copy times
    clip / (norm + 1e-6) (torch.nn.utils.clip_grad_norm_), within the clip kernel's own bound (tests/test_hip_training_kernels.py)"""
    import training_kernels_ref as R
    from oracle import vqgan_oracle as vq
    from test_hip_training_kernels import C
    g, cfg, sd = _tiny()
    x = vq.preprocess_u8(torch.from_numpy(g['frames']))
    tr = _trainer(cfg, sd)
    tr.train_step(x, apply_update=False)
    unclipped = tr.flat_g.cpu().clone()
    norm = float(unclipped.double().norm())
    assert np.isfinite(norm) and norm > 0
    tr.cfg.gradient_clip_val = 0.5 * norm
    tr.apply_gradients()
    torch.cuda.synchronize()
    want, mag = R.clip_grad_norm(unclipped, 0.5 * norm)
    assert abs(float(want.norm()) / norm - 0.5) < 1e-6                          # the reference did clip
    ratio = R.worst_ratio(tr.flat_g.cpu(), want, mag)
    print('clipped flat_g: worst', ratio, 'x 2^-24 x |value|')
    assert ratio <= C['clip_grad_norm_'], ratio


@pytest.mark.parametrize('cfgkw,n', [
    (dict(ch=64, ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[16], image_size=32, z_channels=64, embed_dim=64, n_embed=128), 4),
    (dict(ch=128, ch_mult=[1, 1, 2], num_res_blocks=1, attn_resolutions=[16], image_size=64, z_channels=128, embed_dim=64, n_embed=128), 2),
])
def test_gradients_match_oracle_on_wide_configs(cfgkw, n):
    """channel counts that route the 3x3 convolutions to the split-bf16 halo kernels (Cout % 128 == 0) and all three conv modes"""
    from oracle import vqgan_train_oracle as vt
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.weights import make_vqgan_weights
    cfg = VQGANConfig(perceptual_weight=0.0, codebook_weight=0.7, learning_rate=1e-3, **cfgkw)
    sd = make_vqgan_weights(cfg, seed=11, codebook_scale=1.0)
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(n, 3, cfg.image_size, cfg.image_size)).astype(np.float32))
    tr = _trainer(cfg, sd)
    m = tr.train_step(x, apply_update=False)
    grads, metrics, extra = vt.gradients({k: np.asarray(v) for k, v in sd.items()}, cfg, x)
    assert abs(float(m['total_loss']) - metrics['loss']) < 1e-5 * max(1.0, abs(metrics['loss']))
    same = (tr.last_indices.cpu().view(-1) == extra['ind'].view(-1)).float().mean().item()
    assert same == 1.0, same
    gmax = max(float(v.norm()) for v in grads.values())
    bad = []
    for name in tr.names:
        want = grads[name].numpy()
        got = tr.g(name).cpu().numpy()
        if np.linalg.norm(want) < 1e-7 * gmax:
            if not np.linalg.norm(got) < 1e-5 * gmax:
                bad.append((name, 'nonzero', float(np.linalg.norm(got))))
        elif not _rel(got, want) < 3e-4:
            bad.append((name, _rel(got, want), float(np.linalg.norm(got)), float(np.linalg.norm(want))))
    assert not bad, '\n'.join(map(str, bad))


@pytest.mark.parametrize('n,size', [(2, 32), (3, 64), (2, 128)])
def test_lpips_distance_and_gradient_match_oracle(n, size):
    """perceptual distance (forward) and its gradient w.r.t. the second image vs the fp64 restatement, random VGG/lin weights"""
    from oracle import lpips_oracle as lo
    from viewformer_amd.lpips import LPIPS, make_lpips_weights
    sd = make_lpips_weights(seed=2)
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(n, 3, size, size)).astype(np.float32))
    y = (x + torch.from_numpy(rng.normal(0, 0.2, size=x.shape).astype(np.float32))).clamp(-1, 1)
    net = LPIPS(sd, 'cuda')
    xg, yg = x.permute(0, 2, 3, 1).contiguous().cuda(), y.permute(0, 2, 3, 1).contiguous().cuda()
    got = net(xg, yg).cpu().numpy()
    yo = y.double().requires_grad_(True)
    want = lo.distance(sd, x, yo)
    assert np.allclose(got, want.detach().numpy(), rtol=2e-5, atol=1e-7), (got, want)
    (0.37 * want.sum()).backward()
    p, dy = net.loss_and_grad(xg, yg, 0.37)
    assert np.allclose(p.cpu().numpy(), want.detach().numpy(), rtol=2e-5, atol=1e-7)
    gw = yo.grad.permute(0, 2, 3, 1).numpy()
    # ReLU / max-pool are discontinuous: one unit whose pre-activation rounds to the other side of 0 in fp32 changes the gradient
    # by ~1e-3 of its norm (the fp32 run of the oracle itself is 8.5e-4 away from its fp64 run on the 128 px case), so the fp32
    # restatement is the second admissible reference
    y32 = y.clone().requires_grad_(True)
    (0.37 * lo.distance(sd, x, y32, torch.float32).sum()).backward()
    g32 = y32.grad.permute(0, 2, 3, 1).numpy()
    err = min(_rel(dy.cpu().numpy(), gw), _rel(dy.cpu().numpy(), g32))
    assert err < 1e-4, (err, _rel(dy.cpu().numpy(), gw), _rel(dy.cpu().numpy(), g32))
    # identical images: zero distance
    assert float(net(xg, xg).abs().max()) == 0.0


def test_training_step_with_perceptual_loss_matches_oracle():
    """the reference's default loss (perceptual_weight = 1): L1 + LPIPS + commitment, all gradients vs fp64 autograd"""
    from oracle import vqgan_oracle as vq
    from oracle import vqgan_train_oracle as vt
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.lpips import make_lpips_weights
    from viewformer_amd.weights import make_vqgan_weights
    g = np.load(GOLD)
    cfg = VQGANConfig(ch=32, ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[16], image_size=32, z_channels=32, embed_dim=32,
                      n_embed=64, perceptual_weight=1.0, codebook_weight=1.0, learning_rate=1e-3)
    sd = make_vqgan_weights(cfg, seed=int(g['seed']), codebook_scale=float(g['codebook_scale']))
    lsd = make_lpips_weights(seed=5)
    x = vq.preprocess_u8(torch.from_numpy(g['frames']))
    with pytest.raises(ValueError):
        _trainer(cfg, sd)                                                     # no silent drop of the perceptual term
    tr = _trainer(cfg, sd, lpips_state_dict=lsd)
    m = tr.train_step(x, apply_update=False)
    grads, metrics, extra = vt.gradients({k: np.asarray(v) for k, v in sd.items()}, cfg, x, lpips_sd=lsd)
    assert abs(float(m['total_loss']) - metrics['loss']) < 1e-5 * max(1.0, metrics['loss'])
    assert abs(float(m['p_loss']) - float(extra['p_loss'].detach())) < 1e-5 * max(1.0, float(extra['p_loss'].detach()))
    assert float(m['p_loss']) > 1e-3                                          # the term is live
    gmax = max(float(v.norm()) for v in grads.values())
    bad = []
    for name in tr.names:
        want, got = grads[name].numpy(), tr.g(name).cpu().numpy()
        if np.linalg.norm(want) < 1e-7 * gmax:
            if not np.linalg.norm(got) < 1e-5 * gmax:
                bad.append((name, 'nonzero', float(np.linalg.norm(got))))
        elif not _rel(got, want) < 3e-4:
            bad.append((name, _rel(got, want)))
    assert not bad, '\n'.join(map(str, bad))


@pytest.mark.parametrize('mode,cin,cout,n,h,w', [(1, 128, 128, 2, 16, 16), (1, 256, 64, 1, 8, 32), (2, 128, 256, 2, 32, 32),
                                                 (3, 128, 128, 3, 8, 8), (1, 128, 132, 4, 8, 8)])
def test_conv3_wgrad_kernel_matches_autograd(mode, cin, cout, n, h, w):
    """vf_conv3_wgrad_x6 (weight + bias gradient gathered straight from the NHWC input) vs torch autograd in fp64, the three conv
    modes of the VQGAN (stride 1, pad-right/bottom stride 2, nearest-x2 upsample + stride 1); h, w = INPUT size"""
    import torch.nn.functional as F
    from viewformer_amd import train_ops as T
    rng = np.random.default_rng(mode * 7 + cin)
    x = torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32))
    wt = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    xd = x.double()
    if mode == 1:
        y = F.conv2d(xd, wt, b, padding=1)
    elif mode == 2:
        y = F.conv2d(F.pad(xd, (0, 1, 0, 1)), wt, b, stride=2)                 # Downsample.forward vqgan_th.py:45-49
    else:
        y = F.conv2d(F.interpolate(xd, scale_factor=2.0, mode='nearest'), wt, b, padding=1)      # Upsample.forward :29-32
    ho, wo = y.shape[2], y.shape[3]
    dy = torch.from_numpy(rng.standard_normal((n, cout, ho, wo)).astype(np.float32))
    y.backward(dy.double())
    assert T.conv3_wgrad_supported(cin, n, ho, wo)
    got = T.conv3_wgrad(x.permute(0, 2, 3, 1).contiguous().cuda().view(-1, cin), dy.permute(0, 2, 3, 1).contiguous().cuda().view(-1, cout),
                        n, h, w, cin, ho, wo, cout, mode).cpu().numpy()
    want_w = wt.grad.permute(2, 3, 1, 0).reshape(9 * cin, cout).numpy()       # rows (ky, kx, ci)
    assert _rel(got[:9 * cin], want_w) < 2e-6, _rel(got[:9 * cin], want_w)
    assert _rel(got[9 * cin], b.grad.numpy()) < 2e-6
