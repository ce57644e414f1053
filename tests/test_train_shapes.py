"""The training step's arm decision (viewformer_amd.train.step_plan) at the batch shapes where its row counts stop tiling.

The last block runs on Mx = B (NS - 1) S L rows, every other launch on M = B NS S L.  With NS = 2 and an odd B * S, Mx % 128 == 64; with B * S = 2,
Mx = 128 is under the 256-tile kernels' minimum.  The CPU sweep checks every plan against the conditions the consumers of each fast path state
themselves (ops.*_shape_ok, train_ops.attn_bf16_supported, the bf16 arm of MIGTTrainer._linear_bwd / _linear_dx), separately for the rows each group
of launches runs at.  The GPU cases run one step at such shapes against fp64 autograd over the oracle."""
import numpy as np
import pytest
import torch

from viewformer_amd import ops
from viewformer_amd import train_ops as T
from viewformer_amd.config import MIGTConfig
from viewformer_amd.train import MIGTTrainer, PLAN_SWITCHES, step_plan

SWITCHES_OFF = [None, ('attention_arith', 'f32')] + [(k, False) for k in PLAN_SWITCHES if k != 'attention_arith']


def _cfg(d=768, L=64, n_layer=2):
    return MIGTConfig(d_model=d, n_head=d // 64, n_layer=n_layer, token_image_size=int(round(L ** 0.5)))


def _consumers_accept(cfg, plan, R, r0, rate):
    """what the kernels that read each fast path's operands state about R rows whose first is row r0 of the global batch: a list of the
    plan's flags they refuse (empty: every flag the plan turns on holds at R)"""
    d = cfg.d_model
    layers = [(d, 3 * d), (d, d), (d, 4 * d), (4 * d, d)]
    bad = []
    if (plan.attn16 or plan.act16) and R % 128:                  # a bf16 activation / d(attention output): the bf16 arm of _linear_bwd / _linear_dx
        bad.append('rows16')
    if plan.grad16 and not (R % 128 == 0 and all(ops.gemm_tn_bf16_shape_ok(R, k, n) and ops.gemm_g256_shape_ok(R, n, k) for k, n in layers)):
        bad.append('grad16')
    if plan.gelu_bwd16 and not ops.gemm_g256_shape_ok(R, d, 4 * d):            # mlp.c_proj's dX GEMM: K = d, N = 4 d
        bad.append('gelu_bwd16')
    if plan.u16 and not (plan.gelu_bwd16 and ops.gemm_g256_shape_ok(R, d, 4 * d)):  # a bf16 pre-activation: the 256-tile kernel only
        bad.append('u16')
    if plan.gelu_dual and not (d % 128 == 0 and ops.gemm_g256_shape_ok(R, d, 4 * d)):     # c_fc's dual epilogue: K = d, N = 4 d, 256-tile only
        bad.append('gelu_dual')
    if plan.drop16 and not all(ops.gemm_drop_supported(R, k, n, r0) for k, n in ((d, d), (4 * d, d))):
        bad.append('drop16')
    if plan.res16 and rate and not (r0 % 4 == 0 and ((R + r0 + 3) // 4) * d < 2 ** 32):   # layernorm_bwd(drop=...): 32-bit mask groups
        bad.append('res16')
    return bad


@pytest.mark.parametrize('off', SWITCHES_OFF, ids=lambda o: 'defaults' if o is None else f'{o[0]}={o[1]}')
def test_every_plan_holds_at_the_rows_each_launch_runs_at(off):
    sw = {} if off is None else {off[0]: off[1]}
    tails_kept = tails_dropped = 0
    for d in (128, 384, 768, 1024):
        for L in (16, 64):
            cfg = _cfg(d, L)
            for NS in (2, 3):
                for B in range(1, 9):
                    for S in range(2, 13):
                        M, Mx_pruned, Tn = B * NS * S * L, B * (NS - 1) * S * L, NS * S * L
                        for rate in (0.0, 0.1):
                            for b0 in (0, B):                                  # the first rank, and the second rank's shard of the global batch
                                row0 = b0 * Tn
                                for precision in ('bf16', 'f32'):
                                    plan = step_plan(cfg, precision, B, S, L, NS, rate, row0, **sw)
                                    case = (precision, d, L, NS, B, S, rate, b0, plan)
                                    assert plan.M == M, case
                                    assert plan.Mx == (Mx_pruned if plan.tail else M), case
                                    if plan.attn16:
                                        assert precision == 'bf16' and T.attn_bf16_supported(Tn, L) and d // cfg.n_head == 64, case
                                    if precision == 'f32':
                                        assert not any(plan[3:]), case
                                    assert not _consumers_accept(cfg, plan, M, row0, rate), case
                                    if plan.tail:
                                        assert not _consumers_accept(cfg, plan, plan.Mx, row0 // NS * (NS - 1), rate), case
                                    if not plan.tail:
                                        assert plan.gelu_dual_x == plan.gelu_dual, case
                                    if plan.gelu_dual or plan.gelu_dual_x:
                                        assert plan.act16 and d % 128 == 0, case
                                    if plan.gelu_dual:
                                        assert ops.gemm_g256_shape_ok(M, d, 4 * d), case
                                    if plan.gelu_dual_x:
                                        assert ops.gemm_g256_shape_ok(plan.Mx, d, 4 * d), case
                                    # the prune is given up only where the plan taken at M fails at Mx (not needlessly)
                                    wants_tail = sw.get('prune_last_block', True)
                                    if wants_tail and not plan.tail:
                                        assert _consumers_accept(cfg, plan, Mx_pruned, row0 // NS * (NS - 1), rate), case
                                        tails_dropped += 1
                                    tails_kept += plan.tail
    assert (tails_kept > 0) == sw.get('prune_last_block', True)
    if off is None:
        assert tails_dropped > 0


def _plan(NS, B, S, d=768, L=64, rate=0.0, row0=0, precision='bf16', **sw):
    return step_plan(_cfg(d, L), precision, B, S, L, NS, rate, row0, **sw)


def test_pinned_decisions():
    p = _plan(2, 2, 4)                                           # M 1024, Mx 512: every fast path and the tail
    assert p.tail and p.Mx == 512 and p.attn16 and p.act16 and p.grad16 and p.res16 and p.gelu_dual and p.gelu_dual_x and p.gelu_bwd16
    assert p.u16 and p.gelu_derivative
    p = _plan(2, 1, 3)                                           # M 384, Mx 192 (% 128 == 64): the fast paths at M, no tail
    assert p.grad16 and p.res16 and not p.tail and p.Mx == p.M == 384
    p = _plan(2, 1, 2)                                           # M 256, Mx 128: under the 256-tile minimum
    assert p.grad16 and not p.tail and p.Mx == 256
    p = _plan(3, 1, 2)                                           # Mx 256: exactly at the minimum
    assert p.grad16 and p.tail and p.Mx == 256
    p = _plan(3, 1, 3)                                           # M % 128 == 64: the whole bf16 arm falls back, the tail stays
    assert not p.attn16 and not p.grad16 and p.tail and p.Mx == 384
    p = _plan(2, 1, 3, L=16)                                     # 16-token views: f32 attention
    assert not p.attn16 and p.tail
    for NS, B, S in ((2, 1, 3), (2, 1, 2)):                      # the fp32-equivalent arm prunes at any row count
        p = _plan(NS, B, S, precision='f32')
        assert p.tail and not p.attn16
    p = _plan(3, 1, 2, rate=0.1, row0=384)
    assert p.tail and p.drop16 and p.res16
    p = _plan(3, 2, 4, save_gelu_derivative=False)
    assert p.u16 and not p.gelu_derivative and p.tail
    assert not _plan(2, 2, 4, prune_last_block=False).tail


def test_the_benchmark_step_keeps_the_tail_and_every_fast_path():
    """bench.py --workload train: 10 scenes x 10 views, 3 streams, dropout 0.1, d_model 768"""
    p = _plan(3, 10, 10, rate=0.1)
    assert p.M == 19200 and p.Mx == 12800 and p.tail
    assert all([p.attn16, p.act16, p.grad16, p.res16, p.drop16, p.gelu_dual, p.gelu_dual_x, p.gelu_bwd16, p.u16, p.gelu_derivative]), p
    p = _plan(3, 10, 10, rate=0.1, row0=3 * 19200)                # rank 3 of a data-parallel step
    assert p.tail and p.drop16 and p.res16


def test_step_plan_rejects_unknown_switches():
    with pytest.raises(TypeError):
        _plan(2, 2, 4, fuse_everything=True)


# ------------------------------------------------------------------------------------------------ GPU
BF16_GRAD_TOL = 6e-2        # tests/test_train.py: per-tensor max |grad error| / max |grad| of the bf16 arm against the fp64 oracle


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _err(a, b):
    b = torch.as_tensor(b).double()
    return ((a.detach().cpu().double() - b).abs().max() / (b.abs().max() + 1e-30)).item()


# (arm, NS, B, S, L, dropout, scene_offset, switches, the plan fields the case exists for)
CASES = [
    ('bf16', 2, 2, 4, 64, 0.0, 0, {}, dict(tail=True, Mx=512, grad16=True, res16=True, gelu_bwd16=True, u16=True)),
    ('bf16', 2, 1, 3, 64, 0.0, 0, {}, dict(tail=False, Mx=384, grad16=True, res16=True)),
    ('bf16', 2, 1, 2, 64, 0.0, 0, {}, dict(tail=False, Mx=256, grad16=True, res16=True)),
    ('bf16', 2, 3, 3, 64, 0.0, 0, {}, dict(tail=False, Mx=1152, grad16=True)),
    ('bf16', 3, 1, 2, 64, 0.0, 0, {}, dict(tail=True, Mx=256, grad16=True, res16=True, gelu_dual_x=True)),
    ('bf16', 3, 1, 3, 64, 0.0, 0, {}, dict(tail=True, Mx=384, attn16=False, grad16=False)),
    ('bf16', 3, 2, 4, 64, 0.0, 0, dict(save_gelu_derivative=False), dict(tail=True, Mx=1024, u16=True, gelu_derivative=False)),
    ('bf16', 2, 1, 3, 16, 0.0, 0, {}, dict(tail=True, Mx=48, attn16=False)),
    ('x3h', 2, 1, 3, 64, 0.0, 0, {}, dict(tail=True, Mx=192, attn16=False)),
    ('x3h', 2, 1, 2, 64, 0.0, 0, {}, dict(tail=True, Mx=128, attn16=False)),
    ('x3h', 2, 1, 3, 16, 0.0, 0, {}, dict(tail=True, Mx=48, attn16=False)),
    ('bf16', 2, 1, 3, 64, 0.1, 1, {}, dict(tail=False, drop16=True, res16=True)),
    ('bf16', 3, 1, 2, 64, 0.1, 1, {}, dict(tail=True, Mx=256, drop16=True, res16=True)),
    ('bf16', 2, 2, 4, 64, 0.1, 3, {}, dict(tail=True, Mx=512, drop16=True, res16=True)),
]


def _case_id(c):
    arm, NS, B, S, L, rate, b0, sw, _ = c
    return f'{arm}-NS{NS}-B{B}-S{S}-L{L}' + (f'-drop{rate}-b0{b0}' if rate else '') + ''.join(f'-{k}={v}' for k, v in sw.items())


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[_case_id(c) for c in CASES])
def test_step_at_odd_batch_shapes_against_fp64_autograd(dev, case):
    """one step (no reduction, no update) at d_model 768: the loss and every parameter's gradient against fp64 autograd over the oracle (with
    dropout: the same masks, indexed as the plan prunes)"""
    from oracle import migt_oracle as mg
    from oracle import train_oracle as to
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    arm, NS, B, S, L, rate, b0, sw, want = case
    cfg = MIGTConfig(n_layer=2, sequence_size=S, n_loss_skip=1, token_image_size=int(round(L ** 0.5)), dropout=rate,
                     localization_weight='5' if NS == 3 else '0', pose_multiplier=0.05)
    sd = make_migt_weights(cfg, seed=7, std=0.02)
    g = np.random.Generator(np.random.PCG64(11))
    t = cfg.token_image_size
    tokens = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(B, S, t, t)))
    _, cams = synthetic_scene_batch(B, S, 8, 7)
    poses = mg.normalize_cameras(mg.to_relative_cameras(torch.from_numpy(cams))[0])
    precision = 'bf16' if arm == 'bf16' else 'f32'
    tr = MIGTTrainer(MIGT(cfg, precision=precision, dense_arith='x3h').load_state_dict(sd).to(dev), warmup_steps=4)
    for k, v in sw.items():
        setattr(tr, k, v)
    tr.dropout_seed, tr.step_count, tr.scene_offset = 42, 3, b0
    metrics = tr.train_step(poses, tokens, reduce_gradients=False, apply_update=False)
    torch.cuda.synchronize()
    plan = tr.last_plan
    assert plan == step_plan(cfg, precision, B, S, L, NS, rate, b0 * NS * S * L, **sw)         # the CPU evaluation is the step's own decision
    for k, v in want.items():
        assert getattr(plan, k) == v, (k, plan)
    if rate:
        grads, ref = to.gradients_with_dropout(sd, cfg, poses, tokens, 3, rate, tr.step_seed(3), pruned_last_block=plan.tail, b0=b0)
    else:
        grads, ref = to.gradients(sd, cfg, poses, tokens, step=3)
    loss_tol, grad_tol = (2e-2, BF16_GRAD_TOL) if arm == 'bf16' else (1e-4, 2e-3)
    assert abs(float(metrics['loss']) - ref['loss']) < loss_tol * max(1.0, abs(ref['loss'])), (float(metrics['loss']), ref['loss'])
    worst = ('', 0.0)
    for name in tr.names:
        e = _err(tr.g(name), grads[name].reshape(tr.slices[name][2]))
        worst = max(worst, (name, e), key=lambda w: w[1])
        assert e < grad_tol, (name, e, plan)
    print(_case_id(case), 'worst relative gradient error', worst)


@pytest.mark.gpu
def test_the_benchmark_step_shape_takes_the_tail_and_every_fast_path(dev):
    """bench.py --workload train's shape (3 streams x 10 views x 10 scenes, d_model 768, dropout 0.1) at two layers: what the step really took"""
    from viewformer_amd import geometry
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    B, S = 10, 10
    cfg = MIGTConfig(n_layer=2, sequence_size=S, n_loss_skip=1, localization_weight='5', pose_multiplier=0.05, dropout=0.1)
    tr = MIGTTrainer(MIGT(cfg, precision='bf16').load_state_dict(make_migt_weights(cfg, seed=0)).to(dev))
    g = np.random.Generator(np.random.PCG64(0))
    tokens = torch.from_numpy(g.integers(0, 1024, size=(B, S, 8, 8)))
    _, cams = synthetic_scene_batch(B, S, 8, seed=0)
    poses = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0])
    met = tr.train_step(poses, tokens, reduce_gradients=False, apply_update=False)
    torch.cuda.synchronize()
    p = tr.last_plan
    assert p.M == 19200 and p.Mx == 12800 and p.tail
    assert all([p.attn16, p.act16, p.grad16, p.res16, p.drop16, p.gelu_dual, p.gelu_dual_x, p.gelu_bwd16, p.u16, p.gelu_derivative]), p
    assert torch.isfinite(met['loss']) and bool(torch.isfinite(tr.flat_g).all())
