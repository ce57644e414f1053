"""GPU: the gradient of a photo's log-likelihood with respect to its query camera, from a cached context (DESIGN.md §6.18:
``MIGT.score_grad_from_context``, ``MIGT.refine_from_context``, ``ViewRenderer.score_gradient`` / ``refine``), on both arms.

Exact part: the forward is ``score_from_context``'s, bit for bit, and a view's gradient depends on that view alone — ``torch.equal`` under
a change of N, under chunking, under other views' cameras and codes, for ``n_context = c`` against a cache of c views and for a cache
with NaN in its slack.  Every pass has a multiple of 256 rows (B N a multiple of 4), as in §6.17: the dense layers then take one kernel
whatever the call.  Against the float64 oracle the bound is 8 x the larger of the oracle's own float32 error and the parent route's
relative logit error times the gradient's size — both yardsticks measured here, neither taken from the code under test.  Models are
``SMALL`` of tests/test_hip_score.py (2 layers, d = 128, 2 heads, 128 codes), built as its ``_setup`` builds them; the refinement loop
runs on the same model trained for a second until its logits are peaked (``_trained_setup``)."""
import types

import numpy as np
import pytest
import torch

import score_grad_ref as G
from conftest import parity_report
from test_hip_score import SMALL, SMALL_VQ

pytestmark = pytest.mark.gpu

B_, C_, N_ = 2, 4, 4            # prefill rows 512 (256 for two views), query rows 512
L = 64
SCORE_KEYS = ('token_log_prob', 'log_likelihood', 'predicted_codes', 'confidence', 'entropy', 'accuracy')
_models = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _setup(dev, arm):
    """model, cache, poses and photo codes: built once per arm, shared, left unchanged"""
    from viewformer_amd import geometry
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    if arm not in _models:
        cfg = MIGTConfig(sequence_size=C_ + 1, n_loss_skip=1, localization_weight='1', **SMALL)
        sd = make_migt_weights(cfg, seed=1, std=0.05)
        m = MIGT(cfg, precision=arm).load_state_dict(sd).to(dev)
        g = np.random.Generator(np.random.PCG64(77))
        ctx = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(B_, C_, 8, 8))).to(torch.int32)
        photos = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(B_, 2 * N_, 8, 8))).to(torch.int32).to(dev)
        _, cams = synthetic_scene_batch(B_, C_ + 2 * N_, 8, 78)
        cams = torch.from_numpy(cams)
        p = geometry.normalize_cameras(geometry.to_relative_cameras(cams)[0])
        cpos, qpos = p[:, :C_].contiguous(), p[:, C_:].contiguous().to(dev)
        cache = m.prefill_context(ctx, cpos)
        _models[arm] = types.SimpleNamespace(cfg=cfg, sd=sd, m=m, ctx=ctx, photos=photos, cpos=cpos, qpos=qpos, cams=cams, cache=cache,
                                             full=m.score_grad_from_context(cache, qpos[:, :N_], photos[:, :N_]))
    return _models[arm]


# ---------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_every_shared_key_has_the_bits_of_score_from_context(dev, arm):
    s = _setup(dev, arm)
    want = s.m.score_from_context(s.cache, s.qpos[:, :N_], s.photos[:, :N_], fused=False)
    assert set(s.full) == set(SCORE_KEYS) | {'grad_cameras'} and set(want) == set(SCORE_KEYS)
    for k in SCORE_KEYS:
        assert s.full[k].dtype == want[k].dtype and torch.equal(_bits(s.full[k]), _bits(want[k])), k
    g = s.full['grad_cameras']
    assert g.dtype == torch.float32 and tuple(g.shape) == (B_, N_, 7) and bool(torch.isfinite(g).all()) and bool((g != 0).all())
    again = s.m.score_grad_from_context(s.cache, s.qpos[:, :N_], s.photos[:, :N_])
    assert torch.equal(_bits(again['grad_cameras']), _bits(g))
    empty = s.m.score_grad_from_context(s.cache, s.qpos[:, :0], s.photos[:, :0])
    assert tuple(empty['grad_cameras'].shape) == (B_, 0, 7) and tuple(empty['log_likelihood'].shape) == (B_, 0)
    # one photo per scene against N cameras == the photo repeated
    one = s.m.score_grad_from_context(s.cache, s.qpos[:, :N_], s.photos[:, :1])
    rep = s.m.score_grad_from_context(s.cache, s.qpos[:, :N_], s.photos[:, :1].expand(B_, N_, 8, 8).contiguous())
    assert torch.equal(_bits(one['grad_cameras']), _bits(rep['grad_cameras']))


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_a_views_gradient_depends_on_that_view_alone(dev, arm):
    """N = 4 among N = 8, N = 2 alone, and views 2 ... 3 replaced by other cameras and photos"""
    s = _setup(dev, arm)
    g = s.full['grad_cameras']
    wide = s.m.score_grad_from_context(s.cache, s.qpos, s.photos)                                  # N = 8
    assert torch.equal(_bits(wide['grad_cameras'][:, :N_]), _bits(g))
    two = s.m.score_grad_from_context(s.cache, s.qpos[:, :2], s.photos[:, :2])                     # N = 2: B N = 4
    assert torch.equal(_bits(two['grad_cameras']), _bits(g[:, :2]))
    q2, ph2 = s.qpos[:, :N_].clone(), s.photos[:, :N_].clone()
    q2[:, 2:], ph2[:, 2:] = s.qpos[:, N_ + 2:], s.photos[:, N_ + 2:]
    other = s.m.score_grad_from_context(s.cache, q2, ph2)
    assert torch.equal(_bits(other['grad_cameras'][:, :2]), _bits(g[:, :2]))
    assert not torch.equal(_bits(other['grad_cameras'][:, 2:]), _bits(g[:, 2:]))
    assert torch.equal(_bits(other['grad_cameras'][:, 2:]), _bits(wide['grad_cameras'][:, N_ + 2:]))


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_a_context_length_c_is_a_cache_of_c_views_and_nan_slack_is_not_read(dev, arm):
    s = _setup(dev, arm)
    q, ph = s.qpos[:, :N_], s.photos[:, :N_]
    short = s.m.prefill_context(s.ctx[:, :2], s.cpos[:, :2])
    want = s.m.score_grad_from_context(short, q, ph)
    got = s.m.score_grad_from_context(s.cache, q, ph, n_context=2)
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    assert not torch.equal(_bits(got['grad_cameras']), _bits(s.full['grad_cameras']))             # (the length is not ignored)
    mixed = s.m.score_grad_from_context(s.cache, q, ph, n_context=[[2, 4, 0, 2], [4, 2, 2, 1]])
    sel = torch.tensor([[1, 0, 0, 1], [0, 1, 1, 0]], dtype=torch.bool, device=dev)
    assert torch.equal(_bits(mixed['grad_cameras'][sel]), _bits(want['grad_cameras'][sel]))
    assert torch.equal(_bits(mixed['grad_cameras'][0, 1]), _bits(s.full['grad_cameras'][0, 1]))
    roomy = s.m.prefill_context(s.ctx, s.cpos, capacity=C_ + 2)
    d = s.cfg.d_model
    for kv in roomy.kv:
        kv.view(B_, (C_ + 2) * L, 3 * d)[:, C_ * L:] = float('nan')
    slack = s.m.score_grad_from_context(roomy, q, ph)
    for k in slack:
        assert torch.equal(_bits(slack[k]), _bits(s.full[k])), k


# ---------------------------------------------------------------------------------------------- against the float64 oracle
@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_gradient_against_the_fp64_oracle(dev, arm):
    """C = 2, N = 4, B = 1.  g64: the oracle's gradient; g32: the same oracle in float32 autograd on the CPU; r_fwd: the parent route's
    relative logit error on the same inputs (``generate_from_context(codes_only=False)`` against the float64 logits, over their peak).
    ||g_dev - g64||_inf <= 8 max(||g32 - g64||_inf, r_fwd ||g64||_inf): the backward adds as many rounded launches as the forward has and
    sums 64 token rows per view, whose cancellation neither yardstick sees — a margin over measured yardsticks, not a tuned number."""
    from oracle import migt_oracle as mg
    s = _setup(dev, arm)
    nE = s.cfg.n_embeddings
    C, N = 2, 4
    ctx, cpos, q, ph = s.ctx[:1, :C], s.cpos[:1, :C], s.qpos[:1, :N], s.photos[:1, :N]
    cache = s.m.prefill_context(ctx, cpos)
    g_dev = s.m.score_grad_from_context(cache, q, ph)['grad_cameras'][0].cpu().double()
    g64, _ = G.oracle_grad(s.sd, s.cfg, ctx[0], cpos[0], q[0].cpu(), ph[0].cpu())
    g32, _ = G.oracle_grad(s.sd, s.cfg, ctx[0], cpos[0], q[0].cpu(), ph[0].cpu(), dtype=torch.float32)
    lg = s.m.generate_from_context(cache, q, codes_only=False)[0].cpu().double().view(N, L, nE)
    ids = torch.cat([ctx[0].long(), torch.full_like(ctx[0, :1].long(), nE)], 0)[None]
    l64 = torch.stack([mg.migt_forward(s.sd, s.cfg, ids, torch.cat([cpos[0], q[0, n:n + 1].cpu()], 0)[None], dtype=torch.float64)['logits'][0, -1]
                       for n in range(N)]).view(N, L, nE)
    r_fwd = float((lg - l64).abs().max() / l64.abs().max())
    e_dev, e32, size = float((g_dev - g64).abs().max()), float((g32 - g64).abs().max()), float(g64.abs().max())
    parity_report(test='score_grad_against_fp64_oracle', arm=arm, C=C, N=N, g_dev_minus_g64=e_dev, g32_minus_g64=e32, r_fwd=r_fwd, g64_inf=size,
                  bound=8 * max(e32, r_fwd * size))
    assert e_dev <= 8 * max(e32, r_fwd * size), (e_dev, e32, r_fwd, size)


# ---------------------------------------------------------------------------------------------- refinement
def _perturbed(p, seed):
    """p moved by 0.1 in position and turned by 0.1 rad, each in a seeded random direction"""
    from viewformer_amd import geometry
    g = torch.Generator().manual_seed(seed)
    dx = torch.randn(p.shape[:-1] + (3,), generator=g)
    ax = torch.randn(p.shape[:-1] + (3,), generator=g)
    dx, ax = dx / dx.norm(dim=-1, keepdim=True), ax / ax.norm(dim=-1, keepdim=True)
    dq = torch.cat([torch.full(p.shape[:-1] + (1,), float(np.cos(0.05))), float(np.sin(0.05)) * ax], -1).to(p.device)
    return geometry.normalize_cameras(torch.cat([p[..., :3] + 0.1 * dx.to(p.device), geometry.quaternion_multiply(dq, p[..., 3:])], -1))


def _distance(a, b):
    """(position distance, rotation angle in rad) per view"""
    dot = (a[..., 3:] * b[..., 3:]).sum(-1).abs().clamp(max=1.0)
    return (a[..., :3] - b[..., :3]).norm(dim=-1), 2 * torch.acos(dot)


_trained = {}


def _trained_setup(dev, arm):
    """SMALL trained until its logits are peaked: 8 scenes of 5 views (codes of tests/test_hip_score.py's SMALL_VQ codebook on synthetic
    frames), 300 steps of the bf16 trainer (about a second; ce about 0.01), then loaded into the arm under test with a cache of each
    scene's first 4 views.  The fifth view's pose is the true camera p*: the one pose per scene the head has learnt that photo at."""
    from viewformer_amd import geometry
    from viewformer_amd.config import MIGTConfig, VQGANConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.train import MIGTTrainer
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, make_vqgan_weights, synthetic_scene_batch
    if 'sd' not in _trained:
        B, S = 8, 5
        frames, cams = synthetic_scene_batch(B, S, 32, seed=33)
        vcfg = VQGANConfig(**SMALL_VQ)
        vq = VQGAN(vcfg, data_format='NHWC').load_state_dict(make_vqgan_weights(vcfg, seed=1, codebook_scale=0.05)).to(dev)
        codes = vq.encode(torch.from_numpy(frames.reshape(-1, 32, 32, 3)).to(dev))[-1].view(B, S, 8, 8)
        del vq
        poses = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0])
        cfg = MIGTConfig(sequence_size=S, n_loss_skip=1, localization_weight='1', dropout=0.0, learning_rate=1e-3, weight_decay=0.01,
                         total_steps=2000, **SMALL)
        tr = MIGTTrainer(MIGT(cfg, precision='bf16').load_state_dict(make_migt_weights(cfg, seed=0)).to(dev), warmup_steps=20)
        for _ in range(300):
            met = tr.train_step(poses, codes, reduce_gradients=False)
        _trained.update(sd=tr.state_dict(), cfg=cfg, codes=codes.to(torch.int32), poses=poses, ce=float(met['ce_loss']))
        del tr
    if arm not in _trained:
        t = _trained
        m = MIGT(t['cfg'], precision=arm).load_state_dict(t['sd']).to(dev)
        C = t['codes'].shape[1] - 1
        _trained[arm] = types.SimpleNamespace(m=m, cache=m.prefill_context(t['codes'][:, :C], t['poses'][:, :C].contiguous()),
                                              true=t['poses'][:, C:].contiguous().to(dev), ce=t['ce'])
    return _trained[arm]


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_refinement_never_lowers_the_likelihood(dev, arm):
    """on the trained, peaked model: the photos are what the model renders at the true cameras p*, the start is p* moved by 0.1 and turned
    by 0.1 rad.  Asserted: what the loop guarantees by construction.  Recorded: the distances to p* before and after."""
    s = _trained_setup(dev, arm)
    B_, N_ = s.true.shape[:2]                                                                       # 8 scenes, one view each: 512 rows
    true = s.true
    codes = s.m.generate_from_context(s.cache, true, codes_only=True).to(torch.int32)              # the photos: what the model renders at p*
    start = _perturbed(true, 5)
    r = s.m.refine_from_context(s.cache, start, codes, steps=12, return_trace=True)
    assert {k: tuple(v.shape) for k, v in r.items()} == dict(cameras=(B_, N_, 7), log_likelihood=(B_, N_), initial_log_likelihood=(B_, N_),
                                                            accepted=(B_, N_), trace=(13, B_, N_))
    assert r['accepted'].dtype == torch.int32
    at_start = s.m.score_from_context(s.cache, start, codes)['log_likelihood']
    assert torch.equal(_bits(r['initial_log_likelihood']), _bits(at_start)) and torch.equal(_bits(r['trace'][0]), _bits(at_start))
    assert bool((r['log_likelihood'] >= r['initial_log_likelihood']).all())
    assert bool((r['trace'][1:] >= r['trace'][:-1]).all()) and torch.equal(_bits(r['trace'][-1]), _bits(r['log_likelihood']))
    assert int(r['accepted'].max()) > 0
    assert bool(((r['accepted'] > 0) == (r['log_likelihood'] > r['initial_log_likelihood'])).all())
    at_end = s.m.score_from_context(s.cache, r['cameras'], codes)['log_likelihood']
    assert torch.equal(_bits(at_end), _bits(r['log_likelihood']))                                   # the cameras returned are the ones scored
    q = r['cameras'][..., 3:]
    assert float((q.norm(dim=-1) - 1).abs().max()) < 1e-5 and bool((q[..., 0] >= 0).all())
    twice = s.m.refine_from_context(s.cache, start, codes, steps=12, return_trace=True)
    for k in r:
        assert torch.equal(_bits(twice[k]), _bits(r[k])), k
    on = s.m.refine_from_context(s.cache, r['cameras'], codes, steps=4)
    assert torch.equal(_bits(on['initial_log_likelihood']), _bits(r['log_likelihood']))
    assert bool((on['log_likelihood'] >= r['log_likelihood']).all())
    none = s.m.refine_from_context(s.cache, start, codes, steps=0, return_trace=True)
    assert torch.equal(none['cameras'], start) and tuple(none['trace'].shape) == (1, B_, N_) and int(none['accepted'].sum()) == 0
    (x0, a0), (x1, a1) = _distance(start, true), _distance(r['cameras'], true)
    at_true = s.m.score_grad_from_context(s.cache, true, codes)
    parity_report(test='refine_from_context', arm=arm, steps=12, trained_ce=s.ce, accepted=r['accepted'].flatten().tolist(),
                  log_likelihood_at_true=at_true['log_likelihood'].flatten().tolist(), log_likelihood_before=r['initial_log_likelihood'].flatten().tolist(),
                  log_likelihood_after=r['log_likelihood'].flatten().tolist(), position_error_before=x0.flatten().tolist(),
                  position_error_after=x1.flatten().tolist(), rotation_error_before=a0.flatten().tolist(), rotation_error_after=a1.flatten().tolist(),
                  grad_inf_at_true=float(at_true['grad_cameras'].abs().max()))


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_renderer_gradient_chunks_and_refine(dev, arm):
    from viewformer_amd import geometry
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.render import ViewRenderer, query_poses, refine_views
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_vqgan_weights
    s = _setup(dev, arm)
    vcfg = VQGANConfig(**SMALL_VQ)
    vq = VQGAN(vcfg, data_format='NHWC').load_state_dict(make_vqgan_weights(vcfg, seed=1, codebook_scale=0.05)).to(dev)
    r = ViewRenderer(s.m, vq).set_context(codes=s.ctx, cameras=s.cams[:, :C_])
    world = s.cams[:, C_:].to(dev)                                                                  # 8 cameras, the world frame
    one = r.score_gradient(world, codes=s.photos)
    assert torch.equal(one['poses'], query_poses(world, r.transform))
    direct = s.m.score_grad_from_context(r.cache, one['poses'], s.photos)
    for k in direct:
        assert torch.equal(_bits(one[k]), _bits(direct[k])), k
    for cap in (4, 2):
        for k, v in r.score_gradient(world, codes=s.photos, max_views_per_call=cap).items():
            assert torch.equal(_bits(v), _bits(one[k])), (cap, k)
    plain = r.score(world, codes=s.photos)
    for k in plain:
        assert torch.equal(_bits(plain[k]), _bits(one[k])), k
    # refine: world frame in and out
    photos = s.photos[:, :N_]
    res = r.refine(world[:, :N_], codes=photos, steps=3)
    model = s.m.refine_from_context(r.cache, query_poses(world[:, :N_], r.transform), photos, steps=3)
    for k in model:
        assert torch.equal(_bits(res[k]), _bits(model[k])), k
    assert torch.equal(res['generated_cameras'], geometry.from_relative_cameras(model['cameras'], r.transform))
    halves = r.refine(world[:, :N_], codes=photos, steps=3, max_views_per_call=2, return_trace=True)
    assert tuple(halves['trace'].shape) == (4, B_, N_)
    for k in res:
        assert torch.equal(_bits(halves[k]), _bits(res[k])), k
    # cameras0 = None: the localizer's estimate is the start
    loc = r.localize(codes=photos)['generated_cameras']
    auto, given = r.refine(None, codes=photos, steps=2), r.refine(loc, codes=photos, steps=2)
    for k in auto:
        assert torch.equal(_bits(auto[k]), _bits(given[k])), k
    at_loc = r.score(loc, codes=photos)['log_likelihood']
    assert torch.equal(_bits(auto['initial_log_likelihood']), _bits(at_loc))
    for k, v in refine_views(s.m, vq, None, s.cams[:, :C_], cameras0=loc, codes=s.ctx, photo_codes=photos, steps=2).items():
        assert torch.equal(_bits(v), _bits(given[k])), k


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_the_refinement_loop_does_not_synchronise_with_the_host(dev, arm):
    """under torch's synchronisation check ('error': a blocking copy from the host or a wait for the device raises; a control shows that it
    does): a whole ``refine_from_context`` call on a tight cache with device inputs, and — context lengths being planned on the host and
    copied once, before the first pass — every pass after that preparation (``_score_grad``) with lengths given"""
    if not hasattr(torch.cuda, 'set_sync_debug_mode'):
        pytest.skip('this torch has no sync debug mode')
    from viewformer_amd.render import ascend_poses
    s = _setup(dev, arm)
    q, ph = s.qpos[:, :N_].contiguous(), s.photos[:, :N_].contiguous()
    want = s.m.refine_from_context(s.cache, q, ph, steps=2)                                         # first use: transposed packs, workspaces
    lens = [[2, 4, 0, 2], [4, 2, 2, 1]]
    want_len = s.m.score_grad_from_context(s.cache, q, ph, n_context=lens)
    args = s.m._score_grad_args('test', s.cache, q, ph, lens)                                      # the one copy of the lengths
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.tensor([0.2, 0.2, 0.2, 1.0], device=dev)                                          # the control: a constant built on the host
        got = s.m.refine_from_context(s.cache, q, ph, steps=2)
        got_len = s.m._score_grad(s.cache, *args)
        moved = ascend_poses(q, got_len['grad_cameras'], got['accepted'].float() * 0.01 + 0.01, 0.05)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    for k in want_len:
        assert torch.equal(_bits(got_len[k]), _bits(want_len[k])), k
    assert tuple(moved.shape) == (B_, N_, 7)


def test_refusals(dev):
    from viewformer_amd import _lib
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    s = _setup(dev, 'f32')
    q, ph = s.qpos[:, :N_], s.photos[:, :N_]
    for f in (s.m.score_grad_from_context, s.m.refine_from_context):
        with pytest.raises(ValueError):
            f(s.cache, q[:1], ph)                                                                   # B of another cache
        with pytest.raises(ValueError):
            f(s.cache, q[..., :6], ph)
        with pytest.raises(ValueError):
            f(s.cache, q, ph[:, :3])                                                                # neither N nor 1 photos
        with pytest.raises(ValueError):
            f(s.cache, q, ph.float())
        with pytest.raises(ValueError):
            f(s.cache, q, ph, n_context=C_ + 1)
    for bad in (dict(steps=-1), dict(steps=1.5), dict(step_xyz=0.0), dict(step_rot=float('nan'))):
        with pytest.raises(ValueError):
            s.m.refine_from_context(s.cache, q, ph, **bad)
    other = _setup(dev, 'bf16')
    with pytest.raises(ValueError):
        s.m.score_grad_from_context(other.cache, q, ph)                                             # a foreign cache
    cfg = MIGTConfig(sequence_size=C_ + 1, n_loss_skip=1, localization_weight='1', **SMALL)
    fp8 = MIGT(cfg, precision='bf16', attention='fp8').load_state_dict(make_migt_weights(cfg, seed=1)).to(dev)
    with pytest.raises(_lib.VfError):
        fp8.score_grad_from_context(s.cache, q, ph)
    with pytest.raises(_lib.VfError):
        fp8.refine_from_context(s.cache, q, ph)
