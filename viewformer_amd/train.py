"""One data-parallel training step of the MIGT transformer on MI355X (BASELINE config #4).

Host-side mirror of ``MIGT.train_step`` (viewformer/models/migt.py:464-505): multi-stream forward with saved
activations (streams of :392-401 laid out as extra views, attention by the STREAMS mask), the losses of :416-448
(token cross-entropy on the MASK stream, pose MSE on the LOC stream, views >= n_loss_skip, per-sample means,
``reduce_mean`` over the local batch :476), backward, optional per-tensor ``clip_by_norm`` (:486-487), gradient
all-reduce SUM across replicas (what MirroredStrategy does under ``apply_gradients`` :488 — per-replica mean loss,
summed gradients, no division by the world size) and the AdamWeightDecay update with the warm-up + cosine schedule
of ``create_optimizer`` (viewformer/models/utils.py:371-437,440-564; compile() :457-462 uses 2000 warm-up steps).

All arithmetic is in libvf_hip.so: the backward's dense contractions are vf_igemm_f32 launches
(dX = dY.W^T with transposed-packed weights, dW = X^T.dY through a transpose + packed dY), attention backward
re-materialises the probabilities per head with batched GEMMs (first version: dense, no causal skipping), the rest
are the HBM-bound kernels of csrc/train_ops.hip.  Parameters, gradients and Adam moments live in flat fp32
buffers so that a layer's gradients are one contiguous RCCL all-reduce issued as soon as that layer's backward
is done (overlapping the remaining backward).

Dropout (config.dropout, default 0.1 in the reference: migt.py:72,216,403 and attn_dropout branching_attention.py:15-17) uses a
counter-based mask — keep = hash(seed, site, element index) >= rate * 2^32 (csrc/vf_common.h) — that the backward pass recomputes;
``dropout_seed`` and the step counter give the per-step seed.  The masks cannot coincide with TensorFlow's RNG stream; the tests
check the kernels against autograd with the SAME masks restated in numpy (oracle/train_oracle.py).  In the bf16 arm (the timed one: the
reference trains with --fp16) no dropout site is a pass of its own except the embedding's: the residual / MLP masks are applied by the
epilogue of the projection GEMM (igemm(drop=...)), their backward by the LayerNorm backward that writes the bf16 gradient operand
(layernorm_bwd(drop=...)), the attention's inside the flash forward / backward kernels.

``random_pose_multiplier`` (migt.py:350-354,160-161): each scene's positions are scaled by rpm ** u, u ~ U(-1, 1), on the way in
and the predicted position is divided by the same factor before the loss; u comes from the same counter hash as the dropout masks
(site SITE_POSE_MULT, element = scene index), restated in oracle/train_oracle.py.  ``use_dynamic_pose_loss`` (:107-120,279-284,440):
the learned log-variance pair ``pose_loss_weighting_criterion.pos_ori_weights`` — note the reference SUMS this term over the local
batch (reduce_sum, :117) while every other term is a batch mean; restated as is.
"""
import math
from collections import namedtuple
from typing import NamedTuple

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from . import train_ops as T
from . import geometry
from . import sharding
from .migt import MIGT, _Dense


def parse_schedule(s, total_steps=None):
    """'1', '5.', 'linear(a,b[,N])', 'cosine(a,b[,N])', 'warmup(<inner>,W)' -> callable(step) with ``is_zero()``
    (viewformer/utils/schedules.py:72-248; a missing N is the model's total_steps, migt.py:268)"""
    from .schedules import parse
    sch = parse(s)
    return sch.with_total_steps(total_steps) if total_steps is not None else sch


def learning_rate(step, init_lr, total_steps, warmup_steps, offset: int = 0):
    """WarmUp(CosineDecay) of create_optimizer (models/utils.py:310-361,403-412); ``step`` = optimizer.iterations; ``offset`` = WarmUp.offset
    (models/utils.py:337,341: the schedule counts from there — set by the finetune driver to the restored iteration count)"""
    step = max(step - offset, 0)
    if warmup_steps and step < warmup_steps:
        return init_lr * (step / warmup_steps)
    decay_steps = max(total_steps - warmup_steps, 1)
    t = min(step - warmup_steps, decay_steps)
    return init_lr * 0.5 * (1.0 + math.cos(math.pi * t / decay_steps))


def pose_augmentation_draws(augment: str, n_scenes: int, generator=None, dtype=torch.float32):
    """the random numbers one ``process_batch`` call per scene consumes (train_transformer.py:39-52): a dict of per-scene tensors —
    'shift' [n,3] ~ N(0,1); 'y0' / 'y1' [n] ~ U(0, 2 pi) and 'x' [n] ~ U(0, pi / 8) for 'simple'; 'y0' only for 'advanced'.  The reference draws
    from TensorFlow's global generator, so the stream itself cannot be reproduced — the distributions and their use are what is mirrored."""
    if augment not in ('simple', 'advanced'):
        return {}
    def uni(hi):
        return torch.rand((n_scenes,), generator=generator, dtype=dtype) * hi
    d = dict(shift=torch.randn((n_scenes, 3), generator=generator, dtype=dtype), y0=uni(2 * math.pi))
    if augment == 'simple':
        d.update(x=uni(math.pi / 8), y1=uni(2 * math.pi))
    return d


def process_batch(cameras, tokens, augment: str, split: str, draws=None, generator=None):
    """The token dataset's per-sequence transform (viewformer/train/train_transformer.py:28-61, mapped over every sampled sequence by
    load_token_dataset, data/tfrecord_dataset.py:177-184): ``cameras`` [S,7] or [B,S,7] (xyz + quaternion w,x,y,z) -> the poses the
    model trains on.  'relative': the first view becomes the frame (:31-36); 'no', or any mode outside the training split: unchanged
    (:37-38); 'simple': a random shift and a random rotation Ry * (Rx * Ry) of the whole scene (:39-50); 'advanced': shift + Ry (:51-55);
    then the quaternions are normalised and sign-fixed (:60-61).  One set of random numbers per sequence, as in the reference (its
    shapes are (1, 3) / (1,): broadcast over the sequence's views).  ``draws`` = pose_augmentation_draws(...) to make a call reproducible."""
    cameras = torch.as_tensor(cameras)
    single = cameras.dim() == 2
    cam = cameras[None] if single else cameras
    xyz, quaternion = cam[..., :3], cam[..., 3:]
    if augment == 'relative':
        rotation_inverse = geometry.quaternion_conjugate(quaternion[..., :1, :])
        xyz = geometry.quaternion_rotate(xyz - xyz[..., :1, :], rotation_inverse)
        quaternion = geometry.quaternion_multiply(rotation_inverse, quaternion)
    elif augment == 'no' or split != 'train':
        pass
    elif augment in ('simple', 'advanced'):
        d = draws if draws is not None else pose_augmentation_draws(augment, cam.shape[0], generator, cam.dtype)
        d = {k: v.to(cam.device, cam.dtype) for k, v in d.items()}
        xyz = xyz + d['shift'][:, None, :]
        rotation = geometry.make_quaternion_y(d['y0'])
        if augment == 'simple':
            rotation = geometry.quaternion_multiply(rotation, geometry.quaternion_multiply(geometry.make_quaternion_x(d['x']),
                                                                                            geometry.make_quaternion_y(d['y1'])))
        rotation = rotation[:, None, :]
        xyz = geometry.quaternion_rotate(xyz, rotation)
        quaternion = geometry.quaternion_multiply(quaternion, rotation)
    else:
        raise ValueError(f'Augment {augment} is not supported')
    quaternion = geometry.quaternion_remove_sign(geometry.quaternion_normalize(quaternion))
    out = torch.cat([xyz, quaternion], -1)
    return (out[0] if single else out), tokens


# dropout sites (the `site` word of the counter-based mask): one per Dropout layer instance of the reference
SITE_EMBED = 1
SITE_POSE_MULT = 2                      # per-scene random pose multiplier (host-side draw)
DYN_KEY = 'pose_loss_weighting_criterion.pos_ori_weights'


def site_attn(i):
    return 16 + 4 * i


def site_resid(i):
    return 17 + 4 * i


def site_mlp(i):
    return 18 + 4 * i


def bf16_packed(precision, k, n):
    """the trainer's rule for a dense layer [k][n] with bf16 packings (MIGTTrainer.repack; it drops the model's other packings)"""
    return precision == 'bf16' and k % 128 == 0 and n % 128 == 0


def train_arm(dn, M):
    """the arm of a dense layer's backward launches (dW, dX) at M rows, from the packings repack left in its record: bf16 where both bf16
    packings exist and M % 128 == 0; the split arm 'x6' where both split packings exist (the forward one may be 'x3h': activations
    only) and M % 64 == 0; else native 'f32'.  (The forward launch takes migt.dense_arm(dn) at every M.)"""
    if M % 128 == 0 and 'bf16' in dn.packed and 'bf16' in dn.packed_T:
        return 'bf16'
    split = M % 64 == 0 and 'x6' in dn.packed_T and ('x3h' in dn.packed or 'x6' in dn.packed)
    return 'x6' if split else 'f32'


def block_layer_shapes(cfg):
    """(k, n) of one transformer block's four dense layers (weights.py)"""
    d = cfg.d_model
    return {'attn.c_attn': (d, 3 * d), 'attn.c_proj': (d, d), 'mlp.c_fc': (d, 4 * d), 'mlp.c_proj': (4 * d, d)}


def gelu_dual_ok(cfg, M):
    """c_fc's GELU-dual epilogue at M rows (the 256-tile kernel's limits)"""
    d = cfg.d_model
    return M >= 256 and d % 128 == 0 and (4 * d) % 256 == 0 and M * 4 * d * 2 < 2 ** 31


# the MIGTTrainer switches step_plan reads (their class values are the defaults)
PLAN_SWITCHES = ('attention_arith', 'bf16_saved_activations', 'bf16_gradient_operands', 'tn_weight_gradient', 'bf16_residual_gradient',
                 'fuse_gelu_forward', 'fuse_gelu_backward', 'bf16_preactivation', 'save_gelu_derivative', 'fuse_dropout', 'prune_last_block')


class StepPlan(NamedTuple):
    """what one training step runs (step_plan).  Every flag holds at both row counts the step uses it at: M (the attention, blocks 0 .. n-2)
    and Mx (the last block from its projection on, ln_f)."""
    M: int
    Mx: int                 # M * (NS - 1) / NS with the pruned last block, else M
    tail: bool              # prune_last_block applies
    attn16: bool            # attention on the bf16 pipe; bf16 attention output and d(attention output)
    act16: bool             # LayerNorm outputs / MLP hidden saved as bf16
    grad16: bool            # bf16 gradient operands: TN weight gradients, 256-tile dX GEMMs
    res16: bool             # the LayerNorm backward's bf16 copy of the residual-stream gradient (masked there with dropout)
    drop16: bool            # output dropout in the projection GEMMs' epilogue
    gelu_dual: bool         # c_fc's GELU-dual epilogue at M
    gelu_dual_x: bool       # ... at Mx
    gelu_bwd16: bool        # GELU backward in the epilogue of mlp.c_proj's dX GEMM
    u16: bool               # where the GELU-dual epilogue runs: the pre-activation saved as bf16
    gelu_derivative: bool   # ... holding gelu'(u) instead of u


def step_plan(cfg, precision, B, S, L, NS, rate=0.0, row0=0, **switches):
    """the arm decision of MIGTTrainer.train_step for B scenes of S views, L tokens per view, NS streams, dropout ``rate`` and this rank's
    first row ``row0`` in the global batch — pure host arithmetic on shapes (no device).  ``switches``: PLAN_SWITCHES, default the
    MIGTTrainer class values.  The last block is pruned only where every fast path the plan turns on at M also holds at Mx."""
    sw = {k: switches.pop(k, getattr(MIGTTrainer, k)) for k in PLAN_SWITCHES}
    if switches:
        raise TypeError(f'step_plan: unknown switches {sorted(switches)}')
    d, H = cfg.d_model, cfg.n_head
    Tn, M = NS * S * L, B * NS * S * L
    shapes = block_layer_shapes(cfg)
    p16 = {n: bf16_packed(precision, k, n_) for n, (k, n_) in shapes.items()}
    # attention of the bf16 arm on the bf16 matrix pipe (csrc/attention_dma.hip + attention_train_bf16.hip) where its kernels apply:
    # 64-token views, the wide c_attn / c_proj layers on their bf16 packings; otherwise the exact-f32 kernels.  Attention dropout is
    # inside both sets of kernels (the same masks)
    attn = (sw['attention_arith'] == 'bf16' and precision == 'bf16' and T.attn_bf16_supported(Tn, L) and d // H == 64
            and p16['attn.c_attn'] and p16['attn.c_proj'] and (rate == 0.0 or Tn * (Tn // 4) < 2 ** 32))
    # bf16 arm, wide layers: the activations only GEMMs read — both LayerNorm outputs, the attention output, the MLP hidden — are
    # SAVED AS bf16 by their producers (the rounding the GEMM applied on load before: identical products), so the forward GEMMs take
    # the 256-tile LDS-DMA kernel (bf16 A operand) and the saved activations halve; the backward reads them through the widening
    # transpose (dW) and never otherwise (LayerNorm / GELU backward use the fp32 h / u)
    act = attn and sw['bf16_saved_activations'] and p16['mlp.c_fc'] and p16['mlp.c_proj']

    def at(R, r0):
        """the fast paths R rows (the first of them row r0 of the global batch) can take"""
        # a bf16 operand of a backward GEMM needs the bf16 arm of _linear_bwd / _linear_dx: R % 128 == 0
        attn16 = attn and R % 128 == 0
        act16 = act and R % 128 == 0
        # ... and the two gradients only GEMMs read — d(MLP pre-activation) from the GELU backward, d(q | k | v) from the attention backward —
        # are WRITTEN as bf16 by those kernels (again the rounding their consumers applied on load: identical dX / dW; the bias gradients
        # become sums of the rounded values), so that dX takes the 256-tile kernel and the TN kernel moves half the bytes.  That needs every
        # consumer that can read one: the TN weight-gradient kernel for all four layer shapes of a block (K, N multiples of 256, 32-bit
        # offsets) and the 256-tile GEMM for the dX products (an explicit predicate: d_model 384 or 640 passes the packing rule of `act16`
        # but not these, and keeps fp32 gradients + the transpose / pack weight-gradient path)
        grad16 = (act16 and sw['bf16_gradient_operands'] and sw['tn_weight_gradient']
                  and all(ops.gemm_tn_bf16_shape_ok(R, k, n) and ops.gemm_g256_shape_ok(R, n, k) for k, n in shapes.values()))
        # the LayerNorm backward hands the projection layers' backward GEMMs a bf16 copy of the residual-stream gradient (with dropout: under
        # the consuming layer's output mask, which only the fused form applies there).  With dropout the masks ride in layernorm_bwd(drop=...),
        # which indexes 32-bit mask groups: the same bound gemm_drop_supported puts on the forward — a global batch so large that
        # (R + r0) / 4 * d passes 2^32 falls back to the dropout_add passes instead of raising
        res16 = (grad16 and sw['bf16_residual_gradient'] and sw['fuse_gelu_backward']
                 and (rate == 0.0 or (sw['fuse_dropout'] and r0 % 4 == 0 and ((R + r0 + 3) // 4) * d < 2 ** 32)))
        # residual / MLP dropout in the projection GEMM's epilogue (False: GEMM, then the dropout_add pass: the same masks)
        drop16 = (bool(rate) and sw['fuse_dropout'] and attn16
                  and all(ops.gemm_drop_supported(R, *shapes[n], r0) for n in ('attn.c_proj', 'mlp.c_proj')))
        dual = act16 and sw['fuse_gelu_forward'] and gelu_dual_ok(cfg, R)
        return dict(attn16=attn16, act16=act16, grad16=grad16, res16=res16, drop16=drop16, gelu_dual=dual)

    here = at(M, row0)
    # prune_last_block: the losses read the branch streams only (MASK -> LM head, LOC -> pose head: migt.py:416-448); every block but the last
    # needs the main stream's rows as keys and values of the next one, the LAST block's projection / LayerNorm / MLP on them feed nothing (see
    # MIGTTrainer._block_rows).  Mx = B (NS - 1) S L rows need not tile like M: with NS = 2 and an odd B * S, Mx % 128 == 64; with B * S = 2, Mx = 128 is
    # under the 256-tile kernels' minimum.  The step is pruned only where the plan taken at M holds at Mx as well
    tail = bool(sw['prune_last_block'] and NS > 1 and cfg.n_layer > 0)
    if tail:
        there = at(B * (NS - 1) * S * L, row0 // NS * (NS - 1))
        tail = all(there[k] for k, on in here.items() if on)
    Mx = B * (NS - 1) * S * L if tail else M
    # the pre-activation saved as bf16: its only reader then is the GELU-backward epilogue of the 256-tile kernel, fed by the bf16
    # residual-stream gradient
    u16 = here['res16'] and sw['bf16_preactivation']
    return StepPlan(M=M, Mx=Mx, tail=tail, attn16=here['attn16'], act16=here['act16'], grad16=here['grad16'], res16=here['res16'],
                    drop16=here['drop16'], gelu_dual=here['gelu_dual'],
                    gelu_dual_x=here['act16'] and sw['fuse_gelu_forward'] and gelu_dual_ok(cfg, Mx),
                    gelu_bwd16=here['grad16'] and sw['fuse_gelu_backward'], u16=u16, gelu_derivative=u16 and sw['save_gelu_derivative'])


class Step(NamedTuple):
    """what every phase of one train_step call needs: the shapes, the dropout rate / seed and this rank's position in the global batch,
    the StepPlan.  Built once per step (MIGTTrainer._begin_step)."""
    B: int
    S: int
    L: int
    NS: int                 # streams: main, MASK (, LOC)
    V: int                  # NS * S views per scene
    Tn: int                 # V * L tokens per scene
    M: int                  # B * Tn rows
    M1: int                 # B * S * L rows of one stream
    Mx: int                 # rows from the last block's projection on (StepPlan.Mx)
    rate: float             # 0.0 outside training: Dropout layers are inert with training=False
    seed: int
    row0: int               # this rank's first row ...
    plane0: int             # ... and first attention plane in the global batch
    plan: StepPlan
    training: bool

    def drop(self, site):
        """the dropout tuple of an elementwise site at all M rows"""
        return (self.rate, self.seed, site, self.row0)

    def drop_branch(self, site):
        """... at the Mx rows of the pruned last block and ln_f: the masks there are indexed by the gathered rows"""
        return (self.rate, self.seed, site, self.row0 // self.NS * (self.NS - 1)) if self.plan.tail else self.drop(site)

    def drop_attn(self, i):
        """... of block i's attention weights (a plane offset)"""
        return (self.rate, self.seed, site_attn(i), self.plane0)

    def branch_rows(self, x):
        """the NS - 1 branch streams' rows of x [M][C] (contiguous per scene), gathered: [Mx][C]"""
        return x.view(self.B, self.NS, self.S * self.L, -1)[:, 1:].reshape(self.Mx, -1)

    def scatter_branch_rows(self, x):
        """the inverse for a gradient: back to [M][C] with zeros in the main stream's rows (nothing downstream of them reached a loss)"""
        full = torch.zeros((self.B, self.NS, self.S * self.L, x.shape[-1]), dtype=x.dtype, device=x.device)
        full[:, 1:] = x.view(self.B, self.NS - 1, self.S * self.L, x.shape[-1])
        return full.view(self.M, x.shape[-1])


class BlockSaved(NamedTuple):
    """what a transformer block keeps for its backward"""
    h: torch.Tensor         # the block's input (all M rows)
    n1: torch.Tensor        # ln_1(h)
    qkv: torch.Tensor
    att: torch.Tensor       # the attention output at all rows ...
    att_i: torch.Tensor     # ... and at the rows attn.c_proj ran on (the branch rows in the pruned last block)
    h_mid: torch.Tensor     # h + resid_dropout(c_proj(att))
    n2: torch.Tensor        # ln_2(h_mid)
    u: torch.Tensor         # c_fc's pre-activation (or gelu'(u): u_deriv)
    f: torch.Tensor         # gelu(u)
    lse: torch.Tensor       # the attention's log-sum-exp
    u_deriv: bool


EmbedSaved = namedtuple('EmbedSaved', 'pin u1 h1 ids32 tok rmul')                      # the embedding phase's values for the losses / backward
HeadsSaved = namedtuple('HeadsSaved', 'hmask dlogits lm16 pose')                       # the losses' values for the heads' backward; pose: None or
PoseSaved = namedtuple('PoseSaved', 'hloc up p1 small_n draw')                          # the pose head's


def qkv_thirds(t, d):
    """the (Q, K, V) column thirds of a fused [M][3 d] tensor — stored as (V, Q, K), migt.py:207-213; gradients land in the same thirds —
    and their three leading dimensions"""
    return (t[:, d:2 * d], t[:, 2 * d:], t[:, :d]), (3 * d, 3 * d, 3 * d)


class MIGTTrainer:
    # ------------------------------------------------------------------ switches: the ones step_plan reads, in PLAN_SWITCHES' order ...
    attention_arith = 'bf16'          # bf16 arm only: 'bf16' = attention forward / backward on the bf16 matrix pipe; 'f32' = the exact-f32 kernels
    bf16_saved_activations = True     # bf16 arm: LayerNorm outputs / MLP hidden saved as bf16 (see step_plan); False keeps them fp32 (same gradients)
    bf16_gradient_operands = True     # bf16 arm: gelu_bwd / attention backward write their gradients as bf16 (see step_plan)
    tn_weight_gradient = True         # bf16 arm: dW / db of the wide layers straight from the row-major operands (False: transpose + pack + column sums)
    bf16_residual_gradient = True     # bf16 arm: the LayerNorm backward also writes its result as bf16 — the operand of the two projection
                                      # layers' backward GEMMs, which then run on the 256-tile kernel (the rounding is the one the GEMM's operand
                                      # load applied anyway; only the two bias gradients see it)
    fuse_gelu_forward = True          # bf16 arm: c_fc writes u (fp32, saved) and bf16 gelu(u) from one epilogue (VF_EPI_GELU_DUAL); the GELU there
                                      # is the inference arm's vf_gelu_erf_fast (|err| 1.5e-7: a few outputs round to the neighbouring bf16)
    fuse_gelu_backward = True         # bf16 arm: d(pre-activation) = dX(mlp.c_proj) * gelu'(u) in that GEMM's epilogue (same bits as the two passes)
    bf16_preactivation = True         # bf16 arm, with both GELU fusions: c_fc's pre-activation u is SAVED as bf16 (the reference's mixed_float16 policy
                                      # keeps every activation in half precision); gelu(u) is still taken from the fp32 accumulator, gelu'(u)
                                      # in the backward epilogue from the rounded u.  False: u saved as fp32.
    save_gelu_derivative = True       # bf16 arm, with bf16_preactivation: what c_fc saves for the backward is gelu'(u) (bf16, from the erf / exp evaluation its GELU
                                      # makes anyway: three more instructions per element) instead of u, whose only reader — the GELU-backward epilogue of the
                                      # mlp.c_proj dX GEMM — then multiplies by a loaded value instead of evaluating erf + exp per element again (that epilogue
                                      # was 22 us of a 148 us launch).  gelu' is taken from the fp32 pre-activation and rounded once; before it was evaluated
                                      # on the bf16-rounded u
    fuse_dropout = True               # bf16 arm: residual / MLP dropout in the projection GEMM's epilogue and in the LayerNorm backward's bf16 copy
                                      # (False: the separate dropout_add passes; the same masks, the same values up to the GEMM's own rounding)
    prune_last_block = True           # the last block's projection / LayerNorm / MLP (forward and backward) and ln_f on the branch streams' rows only: the main
                                      # stream's rows of the last block reach no loss (see _block_rows); its dropout masks there are indexed by the gathered rows
    # ... and the rest
    overlap_weight_gradients = True   # bf16 arm: the TN weight-gradient GEMM of a layer on a second stream beside that layer's dX GEMM
    serial_wgrad_split_as_overlapped = False      # (see _weight_gradient)
    early_optimizer = False           # (measured in round 6: 19.660 vs 19.665 ms per step — the update hides, and the backward beside it slows by as much: off)
                                      # bf16 arm: a layer's AdamWeightDecay update and the re-packing of its weights are issued on a third stream as soon as
                                      # that layer's gradients are final (its backward and weight-gradient GEMMs done, its all-reduce complete) — HBM-bound
                                      # work beside the matrix-bound backward of the layers below instead of 0.65 ms at the end of the step.  Same kernels on
                                      # the same values: the parameters after a step are bit-identical (tests/test_train.py)
    fused_optimizer = True            # AdamWeightDecay as ONE launch over the flat buffer (False: one launch per tensor, 468 per step; bit-identical)
    fused_optimizer_repack = True     # bf16 arm: the optimizer step writes the dense layers' bf16 packings from the updated weights in the same pass
                                      # (vf_adamw_flat_pack_f32) instead of a re-pack launch that reads every weight again twice; bit-identical
    one_launch_repack = True          # bf16 arm: all weight packings refreshed by one launch per step
    lazy_gradient_zero = True         # the transformer layers' gradient tensors (85 M of the 88 M) are not zero-filled at the start of a step: each is written
                                      # exactly once per step, so its first writer STORES (sum_slabs / LayerNorm backward with accumulate off) instead of adding
                                      # to a zero — one 337 MB fill and one 337 MB read of zeros less per step.  Keys still unset when a layer's (or the
                                      # step's) backward ends are zero-filled then, so a tensor no kernel wrote is a zero gradient, as before.  The head range
                                      # (embeddings, pose heads, ln_f: several contributions each) is zero-filled as before.  Same bits: x + 0 == x.
    small_n_pose_head = True          # the pose head's 1536 -> 7 layer and its dW on the one-pass small-N kernels (False: the implicit-GEMM kernel, round 5)
    bf16_lm_head = True               # bf16 arm: the tied LM head (logits, dH, dwte) on the bf16 pipe like every other wide layer (the native-f32
                                      # GEMMs it replaces were 0.8 ms of a 21 ms step); False: native f32 MFMA
    attention_backward = 'flash'      # 'dense': the first version (P materialised per head with batched GEMMs), kept for A/B
    scene_offset = None               # index of this rank's first scene in the GLOBAL batch of a data-parallel step (None: rank * local batch).
                                      # Every random draw of the step — the dropout masks, the random pose multiplier — is a function of
                                      # the GLOBAL scene index, so N ranks draw exactly what one process draws on the concatenated batch,
                                      # and no two replicas share a mask (with one seed per step and local indices they all would)
    grad_allreduce_dtype = 'f32'      # 'bf16': each range is all-reduced as a bf16 copy (177 MB instead of 354 MB on the links; the sum
                                      # of the replicas' gradients is then rounded to 8 bits per replica term — an option, off by default:
                                      # the reference's MirroredStrategy reduces fp32 variables' gradients in fp32)
    time_allreduce = False            # record HIP events around the wait for the collectives (exposed_allreduce_ms())
    # ------------------------------------------------------------------ what the trainer caches between steps
    _pack16 = None                    # the one-launch refresh of every bf16 packing (ops.pack_bf16_multi's closure), _pack16_keep its tensors,
    _pack16_keep = None               # _adam_pack the same packings as destinations of the fused optimizer, _layer_pack_ranges the table's
    _adam_pack = None                 # descriptor range per transformer layer (_build_pack_tables)
    _layer_pack_ranges = None
    _packs_fresh = False              # apply_gradients' fused optimizer wrote the packings with the update: the next repack skips them
    _lm_T_stale = True                # _head.packed_T['f32'] is not of the current weights (_pack_lm_T)
    _side_busy = False                # a weight-gradient GEMM is in flight on the 'side' stream (_join_side)
    _unset = frozenset()              # lazy_gradient_zero: the layer tensor pairs no kernel has written yet this step
    _layer_grad_keys = None
    _allreduce_events = None
    last_plan = None                  # the StepPlan of the last train_step call

    def __init__(self, model: MIGT, warmup_steps: int = 2000, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-8, process_group=None):
        cfg = model.config
        if not 0.0 <= cfg.dropout < 1.0:
            raise ValueError('dropout must be in [0, 1)')
        self.dropout_seed = 0
        if not cfg.random_pose_multiplier > 0:
            raise ValueError('random_pose_multiplier must be positive')
        if cfg.use_dynamic_pose_loss and DYN_KEY not in (model._sd_host or {}):
            raise RuntimeError(f'Missing keys: {DYN_KEY} (use_dynamic_pose_loss)')
        if model._sd_host is None or model.device is None:
            raise RuntimeError('load_state_dict() and .to("cuda") the model first')
        self.model, self.cfg, self.dev = model, cfg, model.device
        self.warmup_steps, self.b1, self.b2, self.eps = warmup_steps, beta1, beta2, eps
        self.group = process_group
        self.step_count = 0                          # optimizer.iterations == model._train_counter
        self.lr_offset = 0                           # WarmUp.offset (models/utils.py:337): begin_finetune() moves it
        self.lr_init, self.lr_total_steps = cfg.learning_rate, cfg.total_steps     # create_optimizer's arguments (train_transformer.py)
        self.loc_weight = parse_schedule(cfg.localization_weight, cfg.total_steps)
        self._head = _Dense(cfg.d_model, cfg.n_embeddings)   # the TRAINER's packings of the tied LM head (bf16 both ways, native transposed): the model's own head keeps the native one
        self._streams, self._nodecay = {}, {}            # _stream(name), _nodecay_table(a, b)
        self._layout()
        self._bind()

    # ------------------------------------------------------------------ flat parameter storage
    def _layout(self):
        h, c = self.model._sd_host, self.cfg
        head = ['wte.weight', 'wpe.embeddings']
        for n in ('pose_embedding.c_fc', 'pose_embedding.c_proj', 'pose_criterion.pose_classifier.c_fc',
                  'pose_criterion.pose_classifier.c_proj'):
            head += [n + '.weight', n + '.bias']
        head += ['ln_f.gamma', 'ln_f.beta']
        if c.use_dynamic_pose_loss and self.model.use_localization:
            head.append(DYN_KEY)
        layers = []
        for i in range(c.n_layer):
            p = f'h.{i}'
            names = [p + '.ln_1.gamma', p + '.ln_1.beta', p + '.attn.c_attn.weight', p + '.attn.c_attn.bias',
                     p + '.attn.c_proj.weight', p + '.attn.c_proj.bias', p + '.ln_2.gamma', p + '.ln_2.beta',
                     p + '.mlp.c_fc.weight', p + '.mlp.c_fc.bias', p + '.mlp.c_proj.weight', p + '.mlp.c_proj.bias']
            layers.append(names)
        self.names = head + [n for l in layers for n in l]
        self.slices, off = {}, 0
        for n in self.names:
            shape = tuple(h[n].shape)
            k = int(np.prod(shape))
            self.slices[n] = (off, off + k, shape)
            off += (k + 127) // 128 * 128                # every tensor starts on a 512-byte boundary (float4 kernels need 16; the fused optimizer's
                                                         # 16 x 128 tiles write whole 128-byte lines only when a matrix row starts on one — with the
                                                         # 7-wide pose tensors in front, 16-byte alignment left every tile edge a shared line)
        self.total = off
        self.head_range = (0, self.slices[layers[0][0]][0] if layers else off)
        self.layer_ranges = [(self.slices[l[0]][0], self.slices[l[-1]][1]) for l in layers]
        dev = self.dev
        self.flat_p = torch.zeros(self.total, dtype=torch.float32, device=dev)
        for n in self.names:
            a, b, _ = self.slices[n]
            self.flat_p[a:b] = torch.from_numpy(h[n].reshape(-1)).to(dev)
        self.flat_g = torch.zeros_like(self.flat_p)
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)
        self._scratch = None                                   # clip scratch (T.clip_scratch), allocated by the first clipped step

    def p(self, name):
        a, b, s = self.slices[name]
        return self.flat_p[a:b].view(s)

    def g(self, name):
        a, b, s = self.slices[name]
        return self.flat_g[a:b].view(s)

    def _bind(self):
        """point the model's tensors at the flat buffer and (re)build every packed weight"""
        m = self.model
        m._wte, m._wpe =self.p('wte.weight'), self.p('wpe.embeddings')
        for name, dn in m._dense.items():
            dn.w_raw, dn.bias = self.p(name + '.weight'), self.p(name + '.bias')
        m._head.w_raw = m._wte[:self.cfg.n_embeddings]
        for name in list(m._ln):
            m._ln[name] = (self.p(name + '.gamma'), self.p(name + '.beta'))
        self.repack()

    def repack(self, early_layers_done: bool = False):
        """refresh every packed form of the (just updated) weights: native-f32 packings always (odd shapes, the LM head, the
        pose heads), and with ``dense_arith='x6'`` the fp32-equivalent split packings the dense layers actually run on —
        forward W, and W^T for dX (x6 GEMMs are ~1.8x the native ones; the packers are a few launches per layer).  ``early_layers_done``
        (apply_gradients): the transformer layers' bf16 packings were refreshed right after their early update"""
        m, nE, d, th = self.model, self.cfg.n_embeddings, self.cfg.d_model, self._head
        bf16 = m.precision == 'bf16'          # the reference trains with --fp16 (mixed_float16): bf16 MFMA, fp32 master weights
        split = None if bf16 or m.dense_arith == 'f32' else m.dense_arith     # 'x3h': forward activations only; dX / dW (gradient magnitudes) stay on x6
        lm16 = bf16 and self.bf16_lm_head and d % 256 == 0 and nE % 256 == 0
        if lm16 and 'bf16' not in th.packed:
            self._pack16 = self._adam_pack = None                # (the LM-head packings join the descriptor table: rebuild it)
        if self._pack16 is not None and (not bf16 or any(
                train_arm(dn, 128) != 'bf16' for dn in m._dense.values() if dn.k % 128 == 0 and dn.n % 128 == 0)):
            # the table holds raw pointers into packings that are gone (the arm was switched to f32 and back, or a layer lost its
            # buffers): never run it against them — rebuild from scratch below
            self._pack16 = self._pack16_keep = self._layer_pack_ranges = self._adam_pack = None
        # bf16 arm: after the first call (which allocates the packings one by one and builds the tables: _build_pack_tables) every layer's W and
        # W^T packing is refreshed by ONE launch over a descriptor table (96 pack launches per step before)
        tables = self._pack16 is not None
        packs_fresh, self._packs_fresh = self._packs_fresh, False
        if tables and not packs_fresh:                            # (fresh: apply_gradients' fused optimizer wrote them with the update)
            if early_layers_done and self._layer_pack_ranges is not None:      # only the rest of the table here
                self._pack16(0, min(a for a, n_ in self._layer_pack_ranges))
                self._pack16(max(a + n_ for a, n_ in self._layer_pack_ranges), None)
            else:
                self._pack16()
        new = []                                                  # (name, source, transposed, packing) of the bf16 packings allocated here
        for name, dn in m._dense.items():
            k32 = dn.k % 32 == 0
            to16 = bf16_packed(m.precision, dn.k, dn.n)
            to6 = split is not None and k32 and dn.k % 64 == 0 and dn.n % 64 == 0
            # the native-f32 packings are refreshed only where no faster arm applies (they were 477 pack launches per step that nothing
            # read: the wide layers run on their bf16 / split packings); the transposed native packing of a wide layer is built on demand
            # in _linear_dx for row counts its arm does not tile.  The record's dicts are replaced: what this rule does not keep is gone
            old, old_T, w = dn.packed, dn.packed_T, dn.w_raw
            dn.packed, dn.packed_T = {}, {}
            if k32 and not (to16 or to6):                                                                     # forward: x @ W
                dn.packed['f32'] = ops.pack(w, dn.k, dn.n, 1, sk=dn.n, sn=1, st=0, out=old.get('f32'))
            if dn.n % 32 == 0 and not (to16 or to6):                                                          # dX = dY @ W^T
                dn.packed_T['f32'] = ops.pack(w, dn.n, dn.k, 1, sk=1, sn=dn.n, st=0, out=old_T.get('f32'))
            if to16 and tables:                                   # (the buffers of the one-launch refresh above)
                dn.packed['bf16'], dn.packed_T['bf16'] = old['bf16'], old_T['bf16']
            elif to16:
                dn.packed['bf16'], dn.packed_T['bf16'] = ops.pack_dense('bf16', w), ops.pack_dense('bf16', w, True)
                new += [(name, w, False, dn.packed['bf16']), (name, w, True, dn.packed_T['bf16'])]
            if to6:
                dn.packed[split] = ops.pack_dense(split, w)
                dn.packed_T['x6'] = ops.pack_dense('x6', w, True)             # [K][N] read as the transposed [N][K] operand
        if lm16 and not tables:                                      # tied LM head on the bf16 pipe: logits = h @ wte^T, dH = dlogits @ wte
            head, first = m._head.w_raw, 'bf16' not in th.packed     # (not the first: the per-tensor refresh, one_launch_repack off)
            th.packed['bf16'], th.packed_T['bf16'] = ops.pack_dense('bf16', head, True), ops.pack_dense('bf16', head)
            if first:
                new += [('wte', head, True, th.packed['bf16']), ('wte', head, False, th.packed_T['bf16'])]
        if bf16 and not tables and new and self.one_launch_repack:
            self._build_pack_tables(new)
        # the model's own head: the fresh native packing and nothing else (logits = h @ wte^T for whoever reads the model afterwards)
        m._head.packed, m._head.packed_T = {'f32': ops.pack(m._wte, d, nE, 1, sk=1, sn=d, st=0, out=m._head.packed.get('f32'))}, {}
        if not lm16:
            self._pack_lm_T()
        else:
            self._lm_T_stale = True           # the step's own predicate also needs M1 % 64 == 0: its fallback must re-pack from THESE weights

    def _build_pack_tables(self, new):
        """the descriptor tables over the bf16 packings ``new`` = [(name, source, transposed, packing)] that repack just allocated (its first
        bf16 call, or the first after the tables were invalidated): from now on _pack16 is the refresh"""
        pack_items = [item[1:] for item in new]
        self._pack16 = ops.pack_bf16_multi(pack_items)          # (re-packs once more)
        self._pack16_keep = pack_items                          # (the closure holds raw pointers: keep the tensors alive with it)
        # the same packings as destinations of the fused optimizer (apply_gradients): one descriptor per weight matrix with both of its
        # packed forms; None when a packing's source is not a whole [rows][cols] view of the flat buffer or a shape does not tile
        by_src, ok = {}, True
        for w, tr, out in pack_items:
            e = by_src.setdefault(w.data_ptr(), [w, None, None])
            ok = ok and e[0].shape == w.shape and e[2 if tr else 1] is None
            e[2 if tr else 1] = out
        nodecay = self._nodecay_table(0, self.total)
        self._adam_pack = T.adamw_pack_table(self.flat_p, [tuple(e) for e in by_src.values()], nodecay) if ok else None
        # descriptor ranges per transformer layer (early_optimizer: a layer's weights are re-packed as soon as they are updated); valid only
        # when every layer's descriptors are contiguous and every wide layer weight is in the table
        rng, ok = [], True
        for i in range(self.cfg.n_layer):
            idx = [j for j, item in enumerate(new) if item[0].startswith(f'h.{i}.')]
            ok = ok and len(idx) == 8 and idx == list(range(idx[0], idx[0] + 8))
            rng.append((idx[0], len(idx)) if idx else (0, 0))
        self._layer_pack_ranges = rng if ok else None

    def _pack_lm_T(self):
        """the tied LM head's native transposed packing (dH = dlogits @ wte), from the current weights"""
        c = self.cfg
        self._head.packed_T['f32'] = ops.pack(self.model._wte, c.n_embeddings, c.d_model, 1, sk=c.d_model, sn=1, st=0, out=self._head.packed_T.get('f32'))
        self._lm_T_stale = False

    def _nodecay_table(self, a, b):
        """device int64 [R][2]: the 'bias' tensors (models/utils.py:424: the only names excluded from the decay) that start inside elements
        [a, b) of the flat buffer, as sorted ranges relative to a — cached per range"""
        if (a, b) not in self._nodecay:
            r = [[s - a, e - a] for s, e in sorted(self.slices[n][:2] for n in self.names if 'bias' in n) if a <= s < b]
            self._nodecay[a, b] = torch.tensor(r, dtype=torch.int64, device=self.dev).reshape(-1, 2)
        return self._nodecay[a, b]

    def _adamw_args(self, a=0, b=None):
        """the arguments of T.adamw_flat_ / adamw_flat_pack_ over elements [a, b) of the flat buffers (default: all of them)"""
        b, wd = self.total if b is None else b, self.cfg.weight_decay
        nodecay = self._nodecay_table(a, b)
        lr, lr_adam = self._adam_scalars()
        return (self.flat_p[a:b], self.flat_g[a:b], self.flat_m[a:b], self.flat_v[a:b], nodecay if wd > 0 else None, lr * wd if wd > 0 else 0.0,
                lr_adam, self.b1, self.b2, self.eps)

    # ------------------------------------------------------------------ building blocks
    def _linear(self, x, name, M, res=None):
        return self.model._gemm(x, name, M, res=res)

    def _proj_dropout(self, x, name, M, res, drop, fused=False):
        """res + dropout(x @ W + b)  (attn.c_proj -> resid_dropout, migt.py:216; mlp.c_proj -> the MLP's dropout, :72).  ``fused``
        (StepPlan.drop16): the mask in the GEMM's epilogue, for a bf16 ``x``"""
        dn = self.model._dense[name]
        if not drop[0]:
            return self._linear(x, name, M, res=res)
        if fused and x.dtype == torch.bfloat16:
            out = torch.empty((M, dn.n), dtype=torch.float32, device=x.device)
            ops.igemm(x, dn.packed['bf16'], M, dn.k, dn.n, out, bias=dn.bias, res=res, bf16=True, a16=True, drop=drop)
            return out
        y = self._linear(x, name, M)
        return T.dropout_add(y, drop[0], drop[1], drop[2], res=res, out=y, row0=drop[3])

    def _linear_bwd(self, name, x, dy, M, need_dx=True, res=None, dx_bf16=False, gelu_bwd_u=None, u_is_derivative=False):
        """grads of y = x @ W + b given dy [M,N]; returns dx (+res) or None.  ``x`` may be a saved bf16 activation (bf16 arm);
        ``dx_bf16``: the bf16 arm's dX GEMM writes bf16 (the attention backward's dO operand); ``gelu_bwd_u``, ``u_is_derivative``: see
        _linear_dx."""
        self._weight_gradient(name, x, dy, M, need_dx)
        return self._linear_dx(name, dy, M, res, dx_bf16, gelu_bwd_u, u_is_derivative) if need_dx else None

    def _weight_gradient(self, name, x, dy, M, dx_follows):
        """dW and db of y = x @ W + b into the layer's gradient pair; ``dx_follows``: the layer's dX GEMM is issued next"""
        dn = self.model._dense[name]
        K, N = dn.k, dn.n
        bf16 = (arm := train_arm(dn, M)) == 'bf16'
        first = self._first_write(name)                   # (lazy_gradient_zero: this layer's gradient pair holds last step's values, not zeros)
        gw, gb = self.g(name + '.weight'), self.g(name + '.bias')
        if bf16 and self.tn_weight_gradient and ops.gemm_tn_bf16_supported(x, M, K, N):
            # bf16 arm with a saved bf16 activation: dW and db in ONE pass over x and dy as they lie (csrc/gemm_tn_bf16.hip) — no widening
            # transpose of x, no packed bf16 copy of dy, no column-sum pass
            if self.overlap_weight_gradients and dx_follows:
                # ... on a SECOND HIP stream, beside the dX GEMM that reads the same dy: both are one under-filled round of 256-tile
                # workgroups (225-243 on 256 CUs, one per CU: 128 KB of LDS each), so the weight gradient's workgroups take the CUs the
                # dX GEMM leaves idle and its tail.  Joined before anything reads the layer's gradients (_join_side)
                side = self._stream('side')
                side.wait_stream(torch.cuda.current_stream(self.dev))                  # dy (and x) are complete
                with torch.cuda.stream(side):
                    ops.gemm_tn_bf16(x, dy, M, K, N, gw, gb, accumulate=not first, beside_another_gemm=True)
                for t in (x, dy):
                    t.record_stream(side)                                              # (the allocator must not recycle them under the side stream)
                self._side_busy = True
            else:
                # (alone on the compute stream the launch takes the full-machine split, another summation order; serial_wgrad_split_as_overlapped
                # keeps the second stream's split, for bit-for-bit comparisons of the two modes)
                ops.gemm_tn_bf16(x, dy, M, K, N, gw, gb, accumulate=not first, beside_another_gemm=self.serial_wgrad_split_as_overlapped and dx_follows)
            return
        if dy.dtype != torch.float32:
            raise RuntimeError('a bf16 gradient operand needs the TN weight-gradient path')
        if first:                                          # the paths below accumulate
            gw.zero_()
            gb.zero_()
        T.colsum(dy, gb, M, N, accumulate=True)
        Mp = (M + 31) // 32 * 32                                                     # reduction length padded to the K stage
        xt = T.transpose(x, M, K, out=torch.zeros((1, K, Mp), dtype=torch.float32, device=x.device) if Mp != M else None, ld_dst=Mp)      # [K][Mp]
        # dW += X^T dY: [K][N] has only (K/128)(N/128) = 36..144 output tiles for 256 CUs but a reduction of M = 19 200 rows -> split-K on
        # the bf16 and x6 arms; the bf16 split count must cut M into whole 64-row chunks of the packing
        tiles = ((K + 127) // 128) * ((N + 127) // 128)
        if bf16:
            want = max(1, min(16, 768 // tiles))
            splits = max([s for s in range(1, want + 1) if M % (64 * s) == 0] or [1])
            if splits > 1 and (K * N) % 4 == 0:
                ops.gemm_bf16_splitk(xt, ops.pack_dense_kn_bf16(dy), K, M, N, gw, splits, lda=Mp)
            else:
                ops.igemm(xt, ops.pack_dense_kn_bf16(dy), K, M, N, gw, res=gw, lda=Mp, bf16=True)
        elif arm == 'x6':
            splits = max(1, min(16, 768 // tiles, M // 1024))
            if splits > 1 and (K * N) % 4 == 0:
                ops.gemm_x6_splitk(xt, ops.pack_dense_kn_x6(dy), K, M, N, gw, splits, lda=Mp)
            else:
                ops.igemm(xt, ops.pack_dense_kn_x6(dy), K, M, N, gw, res=gw, lda=Mp, x6=True)
        else:
            dyp = ops.pack(dy, M, N, 1, sk=N, sn=1, st=0)                            # rows >= M are zero-filled by the packer
            ops.igemm(xt, dyp, K, Mp, N, gw, res=gw, lda=Mp)                         # dW += X^T dY

    def _stream(self, name):
        """the trainer's own HIP streams, created on first use: 'side' (weight-gradient GEMMs beside the dX GEMMs), 'opt' (early_optimizer)"""
        if name not in self._streams:
            self._streams[name] = torch.cuda.Stream(self.dev)
        return self._streams[name]

    def _join_side(self):
        """the compute stream waits for the weight-gradient stream (before a layer's gradients are reduced, clipped or applied)"""
        if self._side_busy:
            torch.cuda.current_stream(self.dev).wait_stream(self._stream('side'))
            self._side_busy = False

    def _adam_scalars(self):
        step = self.step_count
        lr = learning_rate(step, self.lr_init, self.lr_total_steps, self.warmup_steps, self.lr_offset)
        t = step + 1
        return lr, lr * math.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)

    def _early_update_layer(self, i, handle=None):
        """AdamWeightDecay over layer i's range of the flat buffer + its eight bf16 packings, on the optimizer stream"""
        args = self._adamw_args(*self.layer_ranges[i])                       # (the no-decay table is built on the main stream, before the wait below)
        main, opt = torch.cuda.current_stream(self.dev), self._stream('opt')
        opt.wait_stream(main)                                                # the layer's backward (LayerNorm / bias gradients) is queued on main
        if self._side_busy:
            opt.wait_stream(self._stream('side'))                            # ... and its weight-gradient GEMMs + slab sums on the side stream
        with torch.cuda.stream(opt):
            if handle is not None:
                handle.wait()                                                # the layer's gradient all-reduce (this stream waits, not main)
            T.adamw_flat_(*args)
            self._pack16(*self._layer_pack_ranges[i])

    def _linear_dx(self, name, dy, M, res=None, dx_bf16=False, gelu_bwd_u=None, u_is_derivative=False):
        """dx = dy @ W^T (+ res).  ``gelu_bwd_u`` (bf16 arm): the saved pre-activation u of the GELU that produced this layer's input —
        the GEMM's epilogue then returns bf16(dx * gelu'(u)), the GELU backward without the fp32 dx ever reaching HBM.  ``u_is_derivative``
        (save_gelu_derivative): that bf16 tensor holds gelu'(u) already"""
        dn = self.model._dense[name]
        K, N = dn.k, dn.n
        bf16 = (arm := train_arm(dn, M)) == 'bf16'
        if dx_bf16 and not (bf16 and res is None):
            raise RuntimeError('dx_bf16 needs the bf16 arm and no residual')
        dx = torch.empty((M, K), dtype=torch.bfloat16 if dx_bf16 else torch.float32, device=dy.device)
        if gelu_bwd_u is not None:
            if not (bf16 and dx_bf16 and res is None):
                raise RuntimeError('the fused GELU backward needs the bf16 arm, a bf16 result and no residual')
            u16 = gelu_bwd_u.dtype == torch.bfloat16
            ops.igemm(dy, dn.packed_T['bf16'], M, N, K, dx, res=gelu_bwd_u, epilogue=ops.EPI_GELU_BWD, bf16=True, a16=dy.dtype == torch.bfloat16, o16=True,
                      res16=u16, gelu_grad=u16 and u_is_derivative)
        elif bf16:
            ops.igemm(dy, dn.packed_T['bf16'], M, N, K, dx, res=res, bf16=True, a16=dy.dtype == torch.bfloat16, o16=dx_bf16)   # (bf16 dY: the 256-tile kernel)
        elif arm == 'x6':
            ops.igemm(dy, dn.packed_T['x6'], M, N, K, dx, res=res, x6=True)
        else:
            wpT = dn.packed_T.get('f32')
            if wpT is None:                                                          # (a wide layer at a row count its arm does not tile)
                wpT = ops.pack(dn.w_raw, dn.n, dn.k, 1, sk=1, sn=dn.n, st=0)
            ops.igemm(dy, wpT, M, N, K, dx, res=res)
        return dx

    def _begin_gradients(self):
        if not (self.lazy_gradient_zero and self.layer_ranges):
            self.flat_g.zero_()
            self._unset = set()
            return
        if self._layer_grad_keys is None:
            lo = self.layer_ranges[0][0]
            self._layer_grad_keys = ([n[:-7] for n in self.names if n.endswith('.weight') and self.slices[n][0] >= lo and n[:-7] + '.bias' in self.slices]
                                     + [n[:-6] for n in self.names if n.endswith('.gamma') and self.slices[n][0] >= lo and n[:-6] + '.beta' in self.slices])
            covered = sum(self.slices[k + a][1] - self.slices[k + a][0] for k in self._layer_grad_keys
                          for a in (('.weight', '.bias') if k + '.weight' in self.slices else ('.gamma', '.beta')))
            if covered != sum(self.slices[n][1] - self.slices[n][0] for n in self.names if self.slices[n][0] >= lo):
                raise RuntimeError('lazy_gradient_zero: a layer tensor is neither a dense layer\'s weight | bias nor a LayerNorm\'s gamma | beta')
        a, b = self.head_range
        self.flat_g[a:b].zero_()
        self._unset = set(self._layer_grad_keys)

    def _first_write(self, key):
        """True once per step for a layer tensor pair that was not zero-filled: its writer must store, not accumulate"""
        if key in self._unset:
            self._unset.discard(key)
            return True
        return False

    def _flush_unset(self, prefix=''):
        """zero-fill what no kernel wrote (keys under ``prefix``)"""
        for k in [k for k in self._unset if k.startswith(prefix)]:
            for a in (('.weight', '.bias') if k + '.weight' in self.slices else ('.gamma', '.beta')):
                self.g(k + a).zero_()
            self._unset.discard(k)

    def _ln_bwd(self, name, dy, x, M, res=None, also_bf16=False, drop=(0.0, 0, 0)):
        """-> (dx, its bf16 copy under ``drop``'s mask or None)"""
        d = self.cfg.d_model
        dx = T.layernorm_bwd(dy, x, self.p(name + '.gamma'), self.g(name + '.gamma'), self.g(name + '.beta'), M, d, accumulate=not self._first_write(name),
                             res=res, also_bf16=also_bf16, drop=drop if also_bf16 else (0.0, 0, 0))
        return dx if also_bf16 else (dx, None)

    @staticmethod
    def _proj_dy(st, g, g16, drop):
        """the dY of a projection layer whose output went through the dropout site ``drop``, from the residual-stream gradient ``g``: with
        dropout that gradient under the layer's OUTPUT mask — the bf16 copy the LayerNorm backward masked while it wrote it (the fp32 gradient
        stays unmasked), or a dropout_add pass — otherwise the gradient itself"""
        return g16 if st.plan.res16 else T.dropout_add(g, *drop[:3], row0=drop[3]) if drop[0] else g

    def _scene_offset(self, B):
        if self.scene_offset is not None:
            return int(self.scene_offset)
        return (dist.get_rank(self.group) * B) if self._world() > 1 else 0

    def random_pose_factors(self, B, seed, b0=0):
        """rpm ** u_b, u_b = 2 * hash(seed, SITE_POSE_MULT, b0 + b) / 2^32 - 1 (migt.py:351; counter-based like the dropout masks)"""
        from ._hash import dropout_hash
        u = dropout_hash(seed, SITE_POSE_MULT, np.arange(b0, b0 + B, dtype=np.uint64)).astype(np.float64) / 2.0 ** 32 * 2.0 - 1.0
        return torch.from_numpy((float(self.cfg.random_pose_multiplier) ** u).astype(np.float32))

    def step_seed(self, step):
        """per-step dropout seed (uint32) from ``dropout_seed`` and the step counter"""
        return (int(self.dropout_seed) * 0x9E3779B1 + int(step) * 0x85EBCA77 + 0x1234567) & 0xFFFFFFFF

    def _attn_bwd(self, qkv, datt, st, att, lse, drop):
        """dQKV from dA (branching_attention.py:82-126 semantics) with the STREAMS mask.  The bf16 kernels where the plan has them; else
        'flash': one pair of kernels per layer re-materialises the probabilities tile by tile from the saved log-sum-exp and skips masked
        tiles; 'dense': per head with batched GEMMs."""
        d, H = self.cfg.d_model, self.cfg.n_head
        B, Tn, L, spec, attn16 = st.B, st.Tn, st.L, -st.S, st.plan.attn16
        dqkv = torch.empty((st.M, 3 * d), dtype=torch.bfloat16 if attn16 and st.plan.grad16 else torch.float32, device=qkv.device)
        flash = attn16 or self.attention_backward == 'flash'
        if drop[0] and not flash:
            raise NotImplementedError("attention dropout needs attention_backward='flash'")
        if flash:
            thirds, ld = qkv_thirds(qkv, d)
            (T.attn_bwd_bf16 if attn16 else T.attn_bwd)(*thirds, att, datt, lse, *qkv_thirds(dqkv, d)[0], B, H, Tn, L, *ld, d, d, *ld, 1.0, spec, drop=drop)
            return dqkv
        S = torch.empty((B, Tn, Tn), dtype=torch.float32, device=qkv.device)
        dP = torch.empty_like(S)
        pf_T = ops.packed_floats(64, Tn)
        bs = Tn * 3 * d
        for h in range(H):
            q, k, v = qkv[:, d + h * 64:], qkv[:, 2 * d + h * 64:], qkv[:, h * 64:]
            da = datt[:, h * 64:]
            kp = ops.pack(k, 64, Tn, 1, sk=1, sn=3 * d, st=0, batch=B, src_bstride=bs)              # B[c][key] = K[key][c]
            ops.igemm(q, kp, Tn, 64, Tn, S, lda=3 * d, batch=B, stride_x=bs, stride_w=pf_T, stride_out=Tn * Tn)
            T.softmax_mask_(S, B, Tn, L, spec, 1.0)                                                   # P
            vp = ops.pack(v, 64, Tn, 1, sk=1, sn=3 * d, st=0, batch=B, src_bstride=bs)              # B[c][key] = V[key][c]
            ops.igemm(da, vp, Tn, 64, Tn, dP, lda=d, batch=B, stride_x=Tn * d, stride_w=pf_T, stride_out=Tn * Tn)
            T.softmax_mask_bwd_(S, dP, B, Tn, L, spec, 1.0)                                           # dS (in dP)
            pf_k = ops.packed_floats(Tn, 64)
            kq = ops.pack(k, Tn, 64, 1, sk=3 * d, sn=1, st=0, batch=B, src_bstride=bs)              # B[key][c] = K[key][c]
            ops.igemm(dP, kq, Tn, Tn, 64, dqkv[:, d + h * 64:], lda=Tn, ldc=3 * d, batch=B, stride_x=Tn * Tn,
                      stride_w=pf_k, stride_out=bs)                                                   # dQ = dS K
            dSt = T.transpose(dP, Tn, Tn, batch=B, bs_src=Tn * Tn)
            qq = ops.pack(q, Tn, 64, 1, sk=3 * d, sn=1, st=0, batch=B, src_bstride=bs)
            ops.igemm(dSt, qq, Tn, Tn, 64, dqkv[:, 2 * d + h * 64:], lda=Tn, ldc=3 * d, batch=B, stride_x=Tn * Tn,
                      stride_w=pf_k, stride_out=bs)                                                   # dK = dS^T Q
            Pt = T.transpose(S, Tn, Tn, batch=B, bs_src=Tn * Tn)
            dap = ops.pack(da, Tn, 64, 1, sk=d, sn=1, st=0, batch=B, src_bstride=Tn * d)
            ops.igemm(Pt, dap, Tn, Tn, 64, dqkv[:, h * 64:], lda=Tn, ldc=3 * d, batch=B, stride_x=Tn * Tn,
                      stride_w=pf_k, stride_out=bs)                                                   # dV = P^T dA
        return dqkv

    # ------------------------------------------------------------------ the step
    def plan(self, B, S, L, NS, rate=0.0, row0=0):
        """step_plan with this trainer's config, precision and switches"""
        return step_plan(self.cfg, self.model.precision, B, S, L, NS, rate, row0, **{k: getattr(self, k) for k in PLAN_SWITCHES})

    def train_step(self, poses, tokens, reduce_gradients: bool = True, apply_update: bool = True, _forward_only: bool = False):
        """poses [b,S,7] float32 (already through process_batch: relative + normalised), tokens [b,S,t,t] int.
        Returns the metrics dict of MIGT.train_step (loss, ce_loss, acc, pose_* ...).  ``_forward_only`` (test_step / predict_step):
        the same multi-stream graph with ``training=False`` — no dropout, no random pose multiplier — up to the losses; returns
        ``(metrics, outputs)``."""
        poses, tokens = poses.to(self.dev), tokens.to(self.dev)
        st = self._begin_step(poses, tokens, training=not _forward_only)
        # ---- forward with saved activations
        h, emb = self._embed_forward(st, poses, tokens)
        saved = []
        for i in range(self.cfg.n_layer):
            h, rec = self._block_forward(i, h, st)
            if st.training:
                saved.append(rec)
        metrics, outputs, heads = self._losses(st, h, poses, emb)
        if not st.training:
            return metrics, outputs
        # ---- backward; a layer's gradients are reduced (and with early_optimizer applied) as soon as they are final
        overlap, early = self._overlap_plan(reduce_gradients, apply_update)
        dh, dh16 = self._heads_backward(st, h, heads)
        handles = []
        for i in reversed(range(self.cfg.n_layer)):
            dh, dh16 = self._block_backward(i, saved[i], dh, dh16, st)
            saved[i] = None
            hd = None
            if overlap:
                self._join_side()
                hd = self._allreduce_range(*self.layer_ranges[i])
                handles.append(hd)
            if early:
                self._early_update_layer(i, hd[0] if hd is not None else None)
        self._embed_backward(st, dh, emb)
        # ---- clip (per replica, per tensor, before aggregation), all-reduce SUM, AdamWeightDecay
        self._finish_gradients(reduce_gradients, apply_update, overlap, early, handles)
        return metrics

    def _begin_step(self, poses, tokens, training):
        """check the batch, decide the step's arms (step_plan: the bf16 arm's fast paths and the pruned last block, one decision from the shapes,
        valid at every row count it is used at), zero what the gradients need zeroed -> the step's record"""
        c = self.cfg
        if poses.dtype != torch.float32:
            raise TypeError('poses must be float32 (migt.py:346)')
        B, S = tokens.shape[:2]
        L = int(np.prod(tokens.shape[2:]))
        NS = 3 if self.model.use_localization else 2
        if not 0 <= c.n_loss_skip < S:
            raise ValueError('n_loss_skip must be < sequence length')
        if S < 2:
            raise ValueError('train_step needs sequences of at least 2 views (the STREAMS attention mask encodes the stream '
                             'length as -S <= -2; a 1-view sequence has nothing to condition on)')
        if training:
            self._begin_gradients()
        rate = float(c.dropout) if training else 0.0
        b0 = self._scene_offset(B) if rate else 0
        plan = self.last_plan = self.plan(B, S, L, NS, rate, b0 * NS * S * L)
        return Step(B=B, S=S, L=L, NS=NS, V=NS * S, Tn=NS * S * L, M=plan.M, M1=B * S * L, Mx=plan.Mx, rate=rate, seed=self.step_seed(self.step_count),
                    row0=b0 * NS * S * L, plane0=b0 * c.n_head, plan=plan, training=training)

    def _embed_forward(self, st, poses, tokens):
        """the pose embedding MLP and the streams' embeddings (migt.py:392-403) -> (h [M][d], EmbedSaved)"""
        m, c, dev = self.model, self.cfg, self.dev
        B, S, L, d = st.B, st.S, st.L, c.d_model
        rmul = None
        pin = geometry.pose_model_input(poses, c.pose_multiplier)
        if c.random_pose_multiplier != 1 and st.training:                            # migt.py:350-354: rpm ** U(-1, 1) per scene (training only)
            rmul = self.random_pose_factors(B, st.seed, self._scene_offset(B)).to(dev)
            pin = torch.cat([pin[..., :3] * rmul.view(B, 1, 1), pin[..., 3:]], -1)
        pin = pin.reshape(B * S, 7).contiguous()
        fc = m._dense['pose_embedding.c_fc']
        u1 = ops.dense_small_k(pin, fc.w_raw, fc.bias, B * S, 7, fc.n, gelu=False)
        h1 = T.gelu(u1)
        pe = self._linear(h1, 'pose_embedding.c_proj', B * S).view(B, S, d)
        tok = tokens.reshape(B, S, L)
        streams = [(tok, pe), (torch.full_like(tok, m.mask_token), pe)]              # (ids, additive embedding) of the main and the MASK stream
        if st.NS == 3:                                                               # ... and the LOC stream
            streams.append((tok, m._wte[m.localization_token].view(1, 1, d).expand(B, S, d)))
        ids32 = torch.cat([ids for ids, _ in streams], 1).reshape(st.M).to(torch.int32).contiguous()
        add = torch.cat([a for _, a in streams], 1).contiguous().view(B * st.V, d)
        h = ops.embed_sum(ids32, m._wte, m._wpe, add, B * st.V, L, d, c.n_embeddings + 2)
        if st.rate:
            T.dropout_add(h, st.rate, st.seed, SITE_EMBED, out=h, row0=st.row0)      # self.drop, migt.py:403
        return h, EmbedSaved(pin, u1, h1, ids32, tok, rmul)

    def _block_rows(self, i, st):
        """(pruned?, rows, elementwise dropout tuples) of block i from its projection on.  prune_last_block: the losses read the branch streams
        only (MASK -> LM head, LOC -> pose head: migt.py:416-448); every block but the last needs the main stream's rows as keys and values of
        the next one, the LAST block's projection / LayerNorm / MLP on them feed nothing — and their backward multiplies zeros.  From the last
        block's attention on, forward and backward run on the NS - 1 branch streams' rows (Step.branch_rows), ln_f with them; the attention
        backward and everything below it get the two gradients scattered back with zeros in the main stream's rows, which is what they were."""
        last = st.plan.tail and i == self.cfg.n_layer - 1
        return (True, st.Mx, st.drop_branch) if last else (False, st.M, st.drop)

    def _block_forward(self, i, h, st):
        """transformer block i on the residual stream h -> (the stream after it, BlockSaved)"""
        m, d, H, dev, plan, p = self.model, self.cfg.d_model, self.cfg.n_head, self.dev, st.plan, f'h.{i}'
        n1 = ops.layernorm(h, *m._ln[p + '.ln_1'], st.M, d, out_bf16=plan.act16)
        # bf16 arm: c_attn writes q | k | v as bf16, the LDS-DMA kernel of the inference arm (+ log-sum-exp) writes a bf16 output that c_proj
        # reads as it is (the rounding the GEMM would apply on load); otherwise the exact-f32 kernel.  Attention dropout is inside both
        qkv = m._gemm(n1, p + '.attn.c_attn', st.M, out_bf16=True) if plan.attn16 else self._linear(n1, p + '.attn.c_attn', st.M)
        att = torch.empty((st.M, d), dtype=qkv.dtype, device=dev)
        thirds, ld = qkv_thirds(qkv, d)
        lse = (T.attn_fwd_lse_bf16 if plan.attn16 else T.attn_fwd_lse)(*thirds, att, st.B, H, st.Tn, st.L, *ld, d, 1.0, -st.S, drop=st.drop_attn(i))
        last, Mi, drop_i = self._block_rows(i, st)
        att_i, h_i = (st.branch_rows(att), st.branch_rows(h)) if last else (att, h)
        h_mid = self._proj_dropout(att_i, p + '.attn.c_proj', Mi, h_i, drop_i(site_resid(i)), plan.drop16)    # h + resid_dropout(c_proj(a)), migt.py:216,233
        n2 = ops.layernorm(h_mid, *m._ln[p + '.ln_2'], Mi, d, out_bf16=plan.act16)
        u_deriv = False
        if plan.gelu_dual_x if last else plan.gelu_dual:
            # c_fc keeps the pre-activation for the backward pass AND hands bf16 gelu(u) to mlp.c_proj from one epilogue
            dn = m._dense[p + '.mlp.c_fc']
            u = torch.empty((Mi, dn.n), dtype=torch.bfloat16 if plan.u16 else torch.float32, device=dev)
            f = torch.empty((Mi, dn.n), dtype=torch.bfloat16, device=dev)
            u_deriv = plan.gelu_derivative                                            # (`u` then holds gelu'(u): see save_gelu_derivative)
            ops.igemm(n2, dn.packed['bf16'], Mi, dn.k, dn.n, u, bias=dn.bias, epilogue=ops.EPI_GELU_DUAL, bf16=True, a16=True, o16=plan.u16, out_aux=f,
                      gelu_grad=u_deriv)
        else:
            u = self._linear(n2, p + '.mlp.c_fc', Mi)
            f = T.gelu(u, out_bf16=plan.act16)
        h_out = self._proj_dropout(f, p + '.mlp.c_proj', Mi, h_mid, drop_i(site_mlp(i)), plan.drop16)         # h + dropout(mlp(...)), migt.py:72,237
        return h_out, BlockSaved(h, n1, qkv, att, att_i, h_mid, n2, u, f, lse, u_deriv)

    def _losses(self, st, h, poses, emb):
        """ln_f, the token cross-entropy on the MASK stream, the pose MSE on the LOC stream (migt.py:416-448) -> (metrics, the outputs of a
        forward-only step or None, HeadsSaved)"""
        m, c, dev = self.model, self.cfg, self.dev
        B, S, L, M1, d, nE, skip, tok = st.B, st.S, st.L, st.M1, c.d_model, c.n_embeddings, c.n_loss_skip, emb.tok
        so = 1 if st.plan.tail else 0                                                 # (hf's first stream: the main stream is not there when pruned)
        hf = ops.layernorm(h, *m._ln['ln_f'], st.Mx, d).view(B, st.NS - so, S, L, d)
        view_ok = (torch.arange(S, device=dev) >= skip).float().view(1, S, 1).expand(B, S, L).reshape(M1)
        denom = float((S - skip) * L * B)
        hmask = hf[:, 1 - so].contiguous().view(M1, d)
        logits = torch.empty((M1, nE), dtype=torch.float32, device=dev)
        lm16 = 'bf16' in self._head.packed and m.precision == 'bf16' and self.bf16_lm_head and M1 % 64 == 0
        if lm16:
            ops.igemm(hmask, self._head.packed['bf16'], M1, d, nE, logits, bf16=True)
        else:
            ops.igemm(hmask, m._head.packed['f32'], M1, d, nE, logits)
        tgt = tok.reshape(M1).to(torch.int32).contiguous()
        w_ce = (view_ok * (c.image_generation_weight / denom)).contiguous()
        ce_rows, dlogits = T.softmax_ce(logits, tgt, w_ce, M1, nE, c.label_smoothing)        # :420-423
        ce_b = ce_rows.view(B, S, L)[:, skip:].mean((1, 2))
        loss_b = ce_b * c.image_generation_weight
        metrics = dict(ce_loss=ce_b.mean())
        pred = ops.argmax_rows(logits, M1, nE).view(B, S, L)
        metrics['acc'] = (pred[:, skip:] == tok[:, skip:]).float().mean()
        raw = pose = None
        if st.NS == 3:
            pose_term, raw, pose = self._pose_loss(st, hf[:, 2 - so], view_ok, denom, poses, emb.rmul, metrics)
            loss_b = loss_b + pose_term
        metrics['loss'] = loss_b.mean()                                              # reduce_mean, migt.py:476
        outputs = None if st.training else dict(logits=logits.view(B, S, L, nE), predicted_tokens=pred,
                                                pose_head_raw=raw.view(B, S, L, 7) if st.NS == 3 else None)
        return metrics, outputs, HeadsSaved(hmask, dlogits, lm16, pose)

    def _pose_loss(self, st, hloc, view_ok, denom, poses, rmul, metrics):
        """the pose head on the LOC stream's rows ``hloc`` and its MSE (migt.py:432-448); adds its metrics -> (the term of the per-scene loss,
        the head's raw output, PoseSaved)"""
        m, c = self.model, self.cfg
        B, S, L, M1, skip = st.B, st.S, st.L, st.M1, c.n_loss_skip
        loc_w = float(self.loc_weight(self.step_count))
        hloc = hloc.contiguous().view(M1, c.d_model)
        up = self._linear(hloc, 'pose_criterion.pose_classifier.c_fc', M1)
        p1 = T.gelu(up)
        dn_p = m._dense['pose_criterion.pose_classifier.c_proj']
        small_n = self.small_n_pose_head and T.dense_small_n_supported(dn_p.k, dn_p.n) and p1.dtype == torch.float32 and p1.is_contiguous()
        if small_n:          # 1536 -> 7: one pass over p1 instead of an implicit GEMM on a 32-column tile (176 -> ~15 us, round 6)
            raw = T.dense_small_n(p1, dn_p.w_raw, dn_p.bias, M1, dn_p.k, dn_p.n)
        else:
            raw = self._linear(p1, 'pose_criterion.pose_classifier.c_proj', M1)
        dyn = c.use_dynamic_pose_loss
        if dyn:                                                                  # DynamicLossWeightingCriterion, migt.py:107-120
            sw = self.p(DYN_KEY)
            e_pos, e_ori = float(torch.exp(-sw[0])), float(torch.exp(-sw[1]))
            rows_per_scene = float((S - skip) * L)
            w_pos = (view_ok * (loc_w * e_pos / rows_per_scene)).contiguous()    # reduce_SUM over the batch (:117): no 1/B
            w_ori = (view_ok * (loc_w * e_ori / rows_per_scene)).contiguous()
        else:
            w_pos = w_ori = (view_ok * (loc_w / denom)).contiguous()
        div = None if rmul is None else rmul.view(B, 1).expand(B, S * L).reshape(M1).contiguous()
        pos_r, ori_r, draw = T.pose_mse(raw, poses.reshape(B * S, 7).contiguous(), w_pos, M1, L, c.pose_multiplier, w_ori=w_ori, xyz_div=div)
        pos_b = pos_r.view(B, S, L)[:, skip:].mean((1, 2))
        ori_b = ori_r.view(B, S, L)[:, skip:].mean((1, 2))
        if dyn:
            pose_loss = (sw[0] + e_pos * pos_b + sw[1] + e_ori * ori_b).sum()    # a scalar, broadcast onto every scene (:440,447)
            gs = self.g(DYN_KEY)
            gs[0] = loc_w * (B - e_pos * pos_b.sum())
            gs[1] = loc_w * (B - e_ori * ori_b.sum())
            metrics.update(dynamic_loss_weight_pos=sw[0].clone(), dynamic_loss_weight_ori=sw[1].clone(), pose_loss=pose_loss)
        else:
            pose_loss = pos_b + ori_b
            metrics['pose_loss'] = (pos_b + ori_b).mean()
        metrics.update(pose_pos_loss=pos_b.mean(), pose_ori_loss=ori_b.mean(), localization_weight=loc_w)
        return pose_loss * loc_w, raw, PoseSaved(hloc, up, p1, small_n, draw)

    def _heads_backward(self, st, h, heads):
        """the LM head's and the pose head's backward, ln_f's -> the gradient of the last block's output (fp32, bf16 copy or None)"""
        m, c, dev = self.model, self.cfg, self.dev
        B, S, L, M1, d, nE = st.B, st.S, st.L, st.M1, c.d_model, c.n_embeddings
        hmask, dlogits = heads.hmask, heads.dlogits
        so = 1 if st.plan.tail else 0
        dhf = torch.zeros((B, st.NS - so, S, L, d), dtype=torch.float32, device=dev)
        # tied LM head: dH = dlogits @ wte[:nE];  dwte[:nE] = dlogits^T @ H
        dhm = torch.empty((M1, d), dtype=torch.float32, device=dev)
        gwte = self.g('wte.weight')
        if heads.lm16:
            ops.igemm(dlogits, self._head.packed_T['bf16'], M1, nE, d, dhm, bf16=True)
            # dwte[:nE] = dlogits^T @ H straight from the row-major operands (the TN kernel: x = dlogits as bf16, dy = H)
            ops.gemm_tn_bf16(dlogits.to(torch.bfloat16), hmask, M1, nE, d, gwte[:nE], None)
        else:
            if self._lm_T_stale:              # (M1 % 64 != 0 in the bf16 arm: repack() skipped the native transposed packing — build it from the
                self._pack_lm_T()             # CURRENT weights, every step: a packing cached from step 1 would be silently stale)
            ops.igemm(dlogits, self._head.packed_T['f32'], M1, nE, d, dhm)
            M1p = (M1 + 31) // 32 * 32                                                # reduction length padded to the K stage (B * S * L = 48 at
            dlt = T.transpose(dlogits, M1, nE, ld_dst=M1p,                            # 16-token views and an odd B * S)
                              out=torch.zeros((1, nE, M1p), dtype=torch.float32, device=dev) if M1p != M1 else None)
            hp = ops.pack(hmask, M1, d, 1, sk=d, sn=1, st=0)                          # rows >= M1 are zero-filled by the packer
            ops.igemm(dlt, hp, nE, M1p, d, gwte, lda=M1p)                             # rows [0, nE) of the (zeroed) grad
        dhf[:, 1 - so] = dhm.view(B, S, L, d)
        if heads.pose is not None:
            name, (hloc, up, p1, small_n, draw) = 'pose_criterion.pose_classifier.c_proj', heads.pose
            dn = m._dense[name]
            T.colsum(draw, self.g(name + '.bias'), M1, 7, accumulate=True)
            if small_n:          # dW = p1^T @ draw straight from the row-major operands (no transpose, no packing)
                T.dense_small_n_wgrad(p1, draw, self.g(name + '.weight'), M1, dn.k, 7, accumulate=True)
            else:
                p1t = T.transpose(p1, M1, dn.k)
                drp = ops.pack(draw, M1, 7, 1, sk=7, sn=1, st=0)
                ops.igemm(p1t, drp, dn.k, M1, 7, self.g(name + '.weight'))
            w2t = T.transpose(dn.w_raw, dn.k, 7).view(7, dn.k)
            dp1 = ops.dense_small_k(draw, w2t, None, M1, 7, dn.k, gelu=False)
            dup = T.gelu_bwd(up, dp1)
            dhl = self._linear_bwd('pose_criterion.pose_classifier.c_fc', hloc, dup, M1)
            dhf[:, 2 - so] = dhl.view(B, S, L, d)
        nl = c.n_layer
        return self._ln_bwd('ln_f', dhf.view(st.Mx, d), h, st.Mx, also_bf16=st.plan.res16 and nl > 0, drop=st.drop_branch(site_mlp(nl - 1)))

    def _block_backward(self, i, rec, dh, dh16, st):
        """block i's backward from the gradient of its output (fp32 ``dh``, with StepPlan.res16 its bf16 copy under mlp.c_proj's output mask)
        -> the gradient of its input, the same pair for block i - 1"""
        plan, p = st.plan, f'h.{i}'
        last, Mi, drop_i = self._block_rows(i, st)
        dy_mlp = self._proj_dy(st, dh, dh16, drop_i(site_mlp(i)))                    # d(mlp.c_proj output)
        if plan.gelu_bwd16:                                                          # GELU backward in the epilogue of the dX GEMM that feeds it
            du = self._linear_bwd(p + '.mlp.c_proj', rec.f, dy_mlp, Mi, dx_bf16=True, gelu_bwd_u=rec.u, u_is_derivative=rec.u_deriv)
        else:
            df = self._linear_bwd(p + '.mlp.c_proj', rec.f, dy_mlp, Mi)
            du = T.gelu_bwd(rec.u, df, out_bf16=plan.grad16)
        dn2 = self._linear_bwd(p + '.mlp.c_fc', rec.n2, du, Mi)
        dh_mid, dh_mid16 = self._ln_bwd(p + '.ln_2', dn2, rec.h_mid, Mi, res=dh, also_bf16=plan.res16, drop=drop_i(site_resid(i)))   # (+ the residual branch's gradient)
        datt = self._linear_bwd(p + '.attn.c_proj', rec.att_i, self._proj_dy(st, dh_mid, dh_mid16, drop_i(site_resid(i))), Mi, dx_bf16=plan.attn16)
        if last:                             # back to all rows for the attention backward and the block's first half
            datt, dh_mid = st.scatter_branch_rows(datt), st.scatter_branch_rows(dh_mid)
        dqkv = self._attn_bwd(rec.qkv, datt, st, rec.att, rec.lse, st.drop_attn(i))
        dn1 = self._linear_bwd(p + '.attn.c_attn', rec.n1, dqkv, st.M)
        dh, dh16 = self._ln_bwd(p + '.ln_1', dn1, rec.h, st.M, res=dh_mid, also_bf16=plan.res16 and i > 0, drop=st.drop(site_mlp(i - 1)))
        self._flush_unset(p + '.')
        return dh, dh16

    def _embed_backward(self, st, dh, emb):
        """embeddings: dwte scatter, dwpe, d(add) -> pose embedding MLP / LOC token row"""
        m, d = self.model, self.cfg.d_model
        B, S, V, gwte = st.B, st.S, st.V, self.g('wte.weight')
        if st.rate:
            T.dropout_add(dh, st.rate, st.seed, SITE_EMBED, out=dh, row0=st.row0)
        dadd = T.embed_bwd(dh, emb.ids32, gwte, self.g('wpe.embeddings'), B * V, st.L, d, self.cfg.n_embeddings + 2).view(B, V, d)
        dpe = (dadd[:, :S] + dadd[:, S:2 * S]).contiguous().view(B * S, d)
        if st.NS == 3:
            T.colsum(dadd[:, 2 * S:].contiguous().view(B * S, d), gwte[m.localization_token], B * S, d, accumulate=True)
        dh1 = self._linear_bwd('pose_embedding.c_proj', emb.h1, dpe, B * S)
        du1 = T.gelu_bwd(emb.u1, dh1)
        T.dense_small_k_bwd(emb.pin, du1, self.g('pose_embedding.c_fc.weight'), self.g('pose_embedding.c_fc.bias'), B * S, 7,
                            m._dense['pose_embedding.c_fc'].n)

    def _clipped(self):
        return bool(self.cfg.gradient_clip_val and self.cfg.gradient_clip_val > 0)

    def _overlap_plan(self, reduce_gradients, apply_update):
        """(overlap, early): each layer's all-reduce issued as soon as its backward is done; the early per-layer optimizer (see
        early_optimizer), which needs the one-launch optimizer and re-pack tables, no clipping pass over the finished gradients, and — with
        more than one rank — the per-layer fp32 all-reduce whose handle the optimizer stream can wait for"""
        overlap = reduce_gradients and self._world() > 1 and not self._clipped()
        early = (self.early_optimizer and apply_update and self.fused_optimizer and self._pack16 is not None and self._layer_pack_ranges is not None
                 and not self._clipped() and (self._world() == 1 or not reduce_gradients or (overlap and self.grad_allreduce_dtype == 'f32')))
        return overlap, early

    def _finish_gradients(self, reduce_gradients, apply_update, overlap, early, handles):
        c = self.cfg
        self._flush_unset()
        self._join_side()
        if self._clipped():
            if self._scratch is None:
                self._scratch = T.clip_scratch(self.flat_g.device)
            for n in self.names:
                T.clip_by_norm_(self.g(n).reshape(-1), float(c.gradient_clip_val), self._scratch)
        if reduce_gradients and self._world() > 1:
            if overlap:
                handles.append(self._allreduce_range(*self.head_range))
            elif self.grad_allreduce_dtype == 'bf16':
                handles += [self._allreduce_range(a, b) for a, b in [self.head_range] + self.layer_ranges]
            else:
                handles += [(h, None, None) for h in
                            sharding.allreduce_sum_ranges(self.flat_g, [self.head_range] + self.layer_ranges, self.group)]
            ev = None
            if self.time_allreduce:                                                  # what the backward pass did NOT hide: the compute
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))   # stream's wait for the collectives
                ev[0].record()
            for hd, buf, rng in handles:
                hd.wait()
                if buf is not None:                                                  # bf16 bucket: back into the fp32 gradient buffer
                    self.flat_g[rng[0]:rng[1]].copy_(buf)
            if ev is not None:
                ev[1].record()
                self._allreduce_events = ev
        if apply_update:
            self.apply_gradients(layers_done=early)
            if early:
                torch.cuda.current_stream(self.dev).wait_stream(self._stream('opt'))     # the next forward reads the layers' new weights and packings

    def _allreduce_range(self, a, b):
        """async SUM all-reduce of flat_g[a:b] -> (handle, bf16 staging buffer or None, (a, b))"""
        if self.grad_allreduce_dtype == 'bf16':
            buf = self.flat_g[a:b].to(torch.bfloat16)
            return dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True), buf, (a, b)
        return dist.all_reduce(self.flat_g[a:b], op=dist.ReduceOp.SUM, group=self.group, async_op=True), None, (a, b)

    def exposed_allreduce_ms(self):
        """time the compute stream spent waiting for the gradient collectives after the last backward kernel of the most recent step
        (needs ``time_allreduce = True``): what the per-layer overlap did not hide"""
        if self._allreduce_events is None:
            return None
        self._allreduce_events[1].synchronize()
        return self._allreduce_events[0].elapsed_time(self._allreduce_events[1])

    # ------------------------------------------------------------------ evaluation steps (Keras Model.evaluate / predict)
    def test_step(self, poses, tokens, codebook_model=None):
        """``MIGT.test_step`` (migt.py:507-527): the compute_losses graph with ``training=False``, the same loss / accuracy metrics as the
        training step, the pose-head errors, and — given the codebook model — the PSNR of the image decoded from the generated tokens of
        the LAST view against the image decoded from its ground-truth tokens (:521-526)."""
        metrics, out = self.train_step(poses, tokens, _forward_only=True)
        c, skip = self.cfg, self.cfg.n_loss_skip
        if out['pose_head_raw'] is not None:                                         # :514-519 on pose_prediction[:, n_loss_skip:]
            B, S = tokens.shape[:2]
            pp = geometry.pose_head_postprocess(out['pose_head_raw'], c.pose_multiplier)[:, skip:]
            gt = poses.to(self.dev).view(B, S, 1, 7)[:, skip:]
            # AllowNanMean (utils/metrics.py:75-87) as the reference computes it: a NaN sample — asin of a norm that rounding pushed past 1,
            # a zero quaternion — is REPLACED BY 0 and still counted (the weight line :86 tests the already-cleaned values, so no sample is
            # ever dropped): mean over all samples of nan_to_zero(value).  No clamp on the asin argument.
            nan_mean = lambda v: torch.where(torch.isnan(v), torch.zeros_like(v), v).mean()      # noqa: E731
            metrics['pose_pos_err'] = nan_mean((pp[..., :3] - gt[..., :3]).norm(dim=-1))         # CameraPositionError, :90-95
            q1 = geometry.quaternion_normalize(pp[..., 3:])                                     # CameraOrientationError, :98-110: the sine
            q2 = geometry.quaternion_normalize(gt[..., 3:].expand_as(pp[..., 3:]))              # form, stable near zero rotation
            diff = geometry.quaternion_multiply(q1, geometry.quaternion_conjugate(q2))
            metrics['pose_ori_err'] = nan_mean(2.0 * torch.asin(diff[..., 1:].norm(dim=-1)))
        if codebook_model is not None:
            t = c.token_image_size
            gen = out['predicted_tokens'][:, -1].reshape(-1, t, t)
            img = [(codebook_model.decode_code(x.to(torch.int64)).float() / 2 + 0.5).clamp(0, 1) for x in (gen, tokens[:, -1].to(self.dev))]
            mse = ((img[0] - img[1]) ** 2).reshape(img[0].shape[0], -1).mean(1)
            metrics['psnr'] = (10.0 * torch.log10(1.0 / mse.clamp_min(1e-12))).mean()    # tf.image.psnr(max_val=1), batch mean
        return metrics

    def predict_step(self, poses, tokens, codebook_model):
        """``MIGT.predict_step`` (migt.py:532-541): arg-max tokens of every view from the masked stream (special ids -> 0), decoded next
        to the decoded ground-truth tokens."""
        _, out = self.train_step(poses, tokens, _forward_only=True)
        t, nE = self.cfg.token_image_size, self.cfg.n_embeddings
        gen = out['predicted_tokens'].reshape(-1, tokens.shape[1], t, t)
        gen = torch.where(gen < nE, gen, torch.zeros_like(gen))
        dec = codebook_model.decode_code(gen.reshape(-1, t, t).to(torch.int64))
        gt = codebook_model.decode_code(tokens.to(self.dev).reshape(-1, t, t).to(torch.int64))
        return dict(decoded_image=dec, latent_code=gen, ground_truth_image=gt)

    def _world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def apply_gradients(self, layers_done: bool = False):
        """``layers_done``: the transformer layers' ranges were already updated (and re-packed) by train_step's early per-layer optimizer: only the
        head range (embeddings, pose heads, ln_f) is left"""
        c = self.cfg
        if self.fused_optimizer:
            # one launch over the flat buffer (with the early optimizer: over the head range); the "bias" tensors as no-decay ranges
            if layers_done:
                T.adamw_flat_(*self._adamw_args(*self.head_range))
            elif self.fused_optimizer_repack and self._adam_pack is not None and self._pack16 is not None:
                T.adamw_flat_pack_(*self._adamw_args(), self._adam_pack)
                self._packs_fresh = True
            else:
                T.adamw_flat_(*self._adamw_args())
        else:
            lr, lr_adam = self._adam_scalars()
            for n in self.names:
                a, b, _ = self.slices[n]
                decay = c.weight_decay > 0 and 'bias' not in n            # models/utils.py:424: only "bias" names are excluded
                T.adamw_(self.flat_p[a:b], self.flat_g[a:b], self.flat_m[a:b], self.flat_v[a:b],
                         lr * c.weight_decay if decay else 0.0, lr_adam, self.b1, self.b2, self.eps)
        self.step_count += 1
        self.repack(early_layers_done=layers_done)

    def state_dict(self):
        return {n: self.p(n).detach().cpu().clone() for n in self.names}

    # ------------------------------------------------------------------ resume / finetune (the optimizer half of a checkpoint)
    def optimizer_state_dict(self):
        """what ``model.load_weights(checkpoint)`` restores beside the weights (finetune_transformer.py:76-85: "this restores the model and
        the optimizer"): Adam's first / second moments per parameter, optimizer.iterations and the schedule's offset"""
        sd = {'iterations': int(self.step_count), 'lr_offset': int(self.lr_offset)}
        for n in self.names:
            a, b, s = self.slices[n]
            sd['m/' + n] = self.flat_m[a:b].view(s).detach().cpu().clone()
            sd['v/' + n] = self.flat_v[a:b].view(s).detach().cpu().clone()
        return sd

    def load_optimizer_state_dict(self, sd, strict: bool = True):
        want = {p + n for n in self.names for p in ('m/', 'v/')}
        have = {k for k in sd if k.startswith(('m/', 'v/'))}
        if strict and want != have:
            raise RuntimeError(f'optimizer state: missing {sorted(want - have)[:4]}, unexpected {sorted(have - want)[:4]}')
        for n in self.names:
            a, b, s = self.slices[n]
            for pre, flat in (('m/', self.flat_m), ('v/', self.flat_v)):
                if pre + n in sd:
                    t = torch.as_tensor(sd[pre + n], dtype=torch.float32)
                    if tuple(t.shape) != tuple(s):
                        raise RuntimeError(f'optimizer state {pre}{n}: shape {tuple(t.shape)} != {tuple(s)}')
                    flat[a:b] = t.reshape(-1).to(self.dev)
        self.step_count = int(sd.get('iterations', self.step_count))
        self.lr_offset = int(sd.get('lr_offset', self.lr_offset))
        return self

    def begin_finetune(self, learning_rate: float = 1e-5, total_steps: int = None, warmup_steps: int = 2000):
        """viewformer/train/finetune_transformer.py:76-86: a NEW schedule (the finetune learning rate — default 1e-5, :22 — over the finetune
        run's ``total_steps`` with 2000 warm-up steps) on the RESTORED optimizer (moments and iteration count kept: Adam's bias correction goes
        on from the restored count), with the schedule's origin moved to that count (``lr_schedule.offset.assign(optimizer.iterations)``).
        Call after load_state_dict / load_optimizer_state_dict; config overrides (pose_multiplier, localization_weight, ... :57-70) are made
        on the model's config before the trainer is built, as the reference makes them before load_model."""
        self.lr_init = float(learning_rate)          # (the model's config keeps its own total_steps: the localization-weight schedule, migt.py:268)
        if total_steps is not None:
            self.lr_total_steps = int(total_steps)
        self.warmup_steps = int(warmup_steps)
        self.lr_offset = int(self.step_count)
        return self


def finetune_transformer(checkpoint: str, total_steps: int, learning_rate: float = 1e-5, device='cuda', precision: str = 'f32',
                         process_group=None, **transformer_config) -> MIGTTrainer:
    """The model-and-optimizer setup of ``viewformer/train/finetune_transformer.py:57-86`` (the data loop and callbacks around it are the
    caller's): config overrides (pose_multiplier, localization_weight, sequence_size, n_loss_skip, weight_decay, gradient_clip_val,
    augment_poses — only those given) go into ``load_model`` BEFORE the model is built (:57-73); the optimizer is created with the finetune
    learning rate over the finetune run's ``total_steps`` and 2000 warm-up steps, weight decay from the loaded config (:78-82);
    ``model.load_weights(checkpoint).expect_partial()`` restores weights AND optimizer (:84); ``lr_schedule.offset`` is set to the restored
    iteration count (:85).  ``precision='bf16'`` is the driver's ``--fp16`` (:53-55)."""
    from . import checkpoint as ck
    overrides = {k: v for k, v in transformer_config.items() if v is not None}
    model = ck.load_model(checkpoint, device=None, **overrides)
    if not isinstance(model, MIGT):
        raise RuntimeError('finetune_transformer needs a transformer checkpoint')
    if precision != model.precision:
        model = MIGT(model.config, precision=precision).load_state_dict(model._sd_host)
    trainer = MIGTTrainer(model.to(device), process_group=process_group)
    if not checkpoint.endswith(('.pth', '.ckpt')):
        ck.restore_optimizer(trainer, checkpoint, strict=False)             # .expect_partial(): a weights-only checkpoint is accepted
    return trainer.begin_finetune(learning_rate=learning_rate, total_steps=total_steps, warmup_steps=2000)

