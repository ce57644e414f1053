"""7-Scenes localization evaluator on MI355X: the three generation procedures of
viewformer/evaluate/evaluate_sevenscenes.py (``standard``, ``generated_images`` :80-154, ``pose_refinement`` :157-197), the per-scene
loop of its ``main`` (:246-279) and the multi-context variant (evaluate_sevenscenes_multictx.py:36-63), on a ``scene_bank.SceneBank``
in the place of the reference's ``SceneLookup``.

What differs from the reference's data flow, not from its results: context views come from the bank as CODES (a gather; the reference
re-encodes 19 frames per query, and 19 more per refined query), the refinement's search over every training camera is one kernel on
the stream (``ops.camera_knn``; the reference copies the distances to the host and sorts there), and the procedures take B >= 1 queries
per call, each query's result equal to its B = 1 result bit for bit (the reference's loop is batch 1).

Three quirks of the reference are restated literally:
  * ``generate_other_viewpoints`` normalises the offset direction and the rotation axis with ``tf.math.l2_normalize`` WITHOUT an axis
    (:25,:27), i.e. over the whole tensor (sic);
  * ``generated_images`` replaces the LAST ``num_gen_ctx`` views, the target among them (:120-127, sic): from there on the "query" is
    the last generated view;
  * the pose distance takes ``asin`` of a norm that rounding can put above 1; here (host restatement and kernel alike) the argument is
    clamped to 1 — the one deliberate deviation.
"""
import random as _random
from collections import defaultdict

import numpy as np
import torch

from . import _hash
from . import evaluate
from . import evaluate_multictx
from . import geometry
from . import metrics
from . import ops
from .scene_bank import POS_WEIGHT

CONTEXT_SIZE = 19              # the reference's constant (:191,:240)
MAX_OFFSET = 1.0               # :21 "maximum of 1 meter"
MAX_RAD_OFFSET = 0.3           # :22 "maximum rotation difference of 0.3 rad"
SITE_OTHER_VIEWPOINTS = 0x75C  # counter-hash site of generate_other_viewpoints' default draws


def compute_camera_distances(db_cameras, camera, pos_weight: float = POS_WEIGHT):
    """:36-45 on geometry.py's ops (any device): ``db_cameras`` [N,7] against ``camera`` [1,7] (the reference's shape) or any shape that
    broadcasts, e.g. [Q,1,7] -> [Q,N].  The ``asin`` argument is clamped to <= 1 (module docstring).  ``ops.camera_knn`` evaluates the
    same formula in the same operation order."""
    db_cameras, camera = torch.as_tensor(db_cameras), torch.as_tensor(camera)
    d = db_cameras[..., :3] - camera[..., :3]
    pos_distances = torch.sqrt((d * d).sum(-1))                                               # tf.norm, :38
    x1 = geometry.quaternion_normalize(db_cameras[..., 3:])                                   # :39
    x2 = geometry.quaternion_normalize(camera[..., 3:])                                       # :40
    diff = geometry.quaternion_multiply(x1, geometry.quaternion_conjugate(x2))[..., 1:]       # :41
    quat_distances = 2 * torch.asin(torch.sqrt((diff * diff).sum(-1)).clamp(max=1.0))         # :42
    return pos_distances * pos_weight + quat_distances                                        # :45


def default_uniforms(shape, seed: int = 0, site: int = SITE_OTHER_VIEWPOINTS):
    """[*shape, 8] float32 draws in [0, 1) from the project's counter hash (24 bits each: exact in fp32, never 1.0)"""
    n = int(np.prod(shape)) * 8
    h = _hash.dropout_hash(seed, site, np.arange(n, dtype=np.uint64))
    return torch.from_numpy(((h >> np.uint32(8)).astype(np.float32) / np.float32(1 << 24)).reshape(*shape, 8))


def _l2_normalize_all(x, epsilon: float = 1e-12):
    """tf.math.l2_normalize(x) with axis=None: over the WHOLE tensor (sic, :25,:27)"""
    return x * torch.rsqrt(torch.clamp((x * x).sum(), min=epsilon))


def generate_other_viewpoints(camera, uniforms=None, seed: int = 0):
    """:20-33.  ``camera`` [...,7]; ``uniforms`` [...,8] in [0, 1): 3 offset direction, 3 rotation axis, 1 offset length, 1 angle, mapped
    as the reference maps its ``tf.random.uniform`` draws ([-1, 1), [-1, 1), [0, 1 m), [0, 0.3 rad)); default: ``default_uniforms``
    of ``seed``.  Literal (sic): direction and axis are normalised over the whole tensor, not per camera, so with more than one camera
    offsets are shorter than the drawn length and the rotation is smaller than the drawn angle."""
    camera = torch.as_tensor(camera)
    if uniforms is None:
        uniforms = default_uniforms(camera.shape[:-1], seed)
    u = torch.as_tensor(uniforms).to(camera.device, camera.dtype)
    if tuple(u.shape) != tuple(camera.shape[:-1]) + (8,):
        raise ValueError(f'uniforms {tuple(u.shape)}: {tuple(camera.shape[:-1]) + (8,)} expected')
    pos_offset = _l2_normalize_all(u[..., 0:3] * 2 - 1)                                       # :24-25
    quaternion_axis = _l2_normalize_all(u[..., 3:6] * 2 - 1)                                  # :26-27
    pos_offset = pos_offset * (u[..., 6:7] * MAX_OFFSET)                                      # :28
    angle = u[..., 7:8] * MAX_RAD_OFFSET                                                      # :29
    quaternion_rot = torch.cat((torch.cos(angle / 2), torch.sin(angle / 2) * quaternion_axis), -1)   # :30
    xyz, quaternion = camera[..., :3], camera[..., 3:]                                        # :31
    return torch.cat((pos_offset + xyz, geometry.quaternion_normalize(geometry.quaternion_multiply(quaternion_rot, quaternion))), -1)


def load_image_match_map(image_match_map_filepath):
    """:71-77: lines of ``<query file> <matched training file>`` -> {query: [matches in file order]}"""
    top_map = defaultdict(list)
    with open(image_match_map_filepath, 'r') as f:
        for line in f:
            fr, to = line.strip('\n\r').split()
            top_map[fr].append(to)
    return top_map


def build_image_match_map(bank, queries, top_n: int, window: int = 0, batch_size: int = 64):
    """The match map the reference reads from an outside retrieval system's file (:71-77), made from the bank itself: ``queries`` yields
    the ``(frames uint8 [1,H,W,3], camera, file)`` items ``evaluate_scene`` takes; -> {file + '.color.png': [the ``top_n`` bank file
    names that look most like the query, nearest first]} (``SceneBank.similar``: the code distance of ``ops.code_knn`` with ``window``),
    ``batch_size`` queries per search.  What ``evaluate_scene(match_map=...)`` and ``load_image_match_map`` use."""
    match_map = {}
    for batch in _batched(queries, batch_size):
        frames = torch.cat([torch.as_tensor(f) for f, _, _ in batch])                          # [B,H,W,3]
        idx = bank.similar(images=frames, k=top_n, window=window).cpu().tolist()
        for (_, _, file), row in zip(batch, idx):
            match_map[file + '.color.png'] = [bank.files[i] for i in row]
    return match_map


def save_image_match_map(path, match_map):
    """write ``match_map`` in the reference's text format, ``<query file> <matched file>`` per line, matches in list order:
    ``load_image_match_map(path)`` returns an equal mapping"""
    with open(path, 'w') as f:
        for query, matches in match_map.items():
            for m in matches:
                if len(query.split()) != 1 or len(m.split()) != 1:
                    raise ValueError(f'file names with white space cannot be written to a match map: {query!r} {m!r}')
                f.write(f'{query} {m}\n')


def draw_fill_indices(bank, count: int, rng=_random):
    """``random.sample(scene_lookup.files, count)`` (:191,:240) as bank indices, drawn on the host"""
    return [bank.index(x) for x in rng.sample(bank.files, count)]


def build_batch(bank, gt_frames, gt_cameras, matches=(), context_size: int = CONTEXT_SIZE, rng=_random, top_n: int = None,
                context_frames: bool = True):
    """``build_batch`` of main (:234-244) for one query: ``gt_frames`` [1,H,W,3], ``gt_cameras`` [1,7]; ``matches``: the query's matched
    training files (they come first, truncated to ``top_n`` when given, :239), the rest of the ``context_size`` views are a
    ``rng.sample`` over the bank's files (:240).  -> (cameras [1,S,7], frames, indices [S-1] into the bank); ``frames`` is [1,S,H,W,3]
    when the bank keeps pixels (and ``context_frames``) and [1,1,H,W,3] (the query alone) otherwise: the code-based procedures read the
    context from the bank."""
    ctx = list(matches)[:top_n] if top_n is not None else list(matches)
    ctx = ctx + rng.sample(bank.files, context_size - len(ctx))
    indices = [bank.index(x) for x in ctx]
    gt_cameras = np.asarray(torch.as_tensor(gt_cameras).cpu(), dtype=np.float32).reshape(1, 7)
    cameras = np.concatenate((bank.cameras_host[indices], gt_cameras), 0)[np.newaxis, ...]                    # :242
    gt_frames = torch.as_tensor(gt_frames)
    if context_frames and getattr(bank, 'frames', None) is not None:
        bank_frames = torch.as_tensor(bank.frames)
        ctx_frames = bank_frames[torch.as_tensor(indices, dtype=torch.long, device=bank_frames.device)]
        frames = torch.cat((ctx_frames, gt_frames.to(bank_frames.device)), 0)[None]                           # :243
    else:
        frames = gt_frames[None]
    return torch.from_numpy(cameras), frames, indices


def _encode(codebook_model, transformer_model, images):
    """the evaluators' ``encode`` helper (:166-177): images uint8 [B,S,H,W,3] on the device -> codes int32 [B,S,t,t]"""
    B, S = images.shape[:2]
    t = transformer_model.config.token_image_size
    frames = evaluate._frames_for_encode(images, codebook_model.config.image_size)
    return codebook_model.encode(frames)[-1].to(torch.int32).view(B, S, t, t)


def _view_codes(bank, transformer_model, codebook_model, images, context_indices, reencode):
    """codes of a batch's S views: the context from the bank when the caller drew it there (only the query frame is encoded), else every
    frame through the encoder"""
    if context_indices is None or reencode:
        return _encode(codebook_model, transformer_model, images)
    ctx = bank.gather(torch.as_tensor(context_indices).reshape(images.shape[0], -1))[0]
    return torch.cat((ctx, _encode(codebook_model, transformer_model, images[:, -1:])), 1)


def _localize(transformer_model, codes, cameras):
    """the localization pass (:180-181): all S code maps, S-1 poses, LOC embedding on the last view -> (camera [B,1,7], head output)"""
    out = transformer_model(dict(input_ids=codes, poses=cameras[:, :-1].contiguous()), training=False, last_view_logits_only=True)
    pose_last = out['pose_prediction'][:, -1:]
    return transformer_model.reduce_cameras(pose_last, -2), pose_last


def generate_batch_predictions_using_pose_refinement(bank, transformer_model, codebook_model, images, cameras, num_gen_ctx: int = 9,
                                                     fill_indices=None, context_size: int = CONTEXT_SIZE, context_indices=None,
                                                     reencode: bool = False, return_intermediates: bool = False, rng=_random):
    """:157-197 for B >= 1 queries.  ``images`` uint8 [B,S,H,W,3] (with ``context_indices`` [B,S-1] — the bank views the caller drew the
    context from, as ``build_batch`` returns them — only the query ``images[:, -1]`` is read and encoded, and ``images`` may be
    [B,1,H,W,3]), ``cameras`` [B,S,7].  First localization pass -> camera in the scene's frame -> the ``num_gen_ctx`` nearest bank views
    (``bank.nearest``: on the device, no host round trip) ++ ``fill_indices`` [B, context_size - num_gen_ctx] (default: a
    ``rng.sample`` over the bank per query as the reference draws it, :191, on the host before anything is launched) -> the standard
    generation on the gathered CODES with the query's own codes and ground-truth camera appended (:195-197).  ``reencode``: take FRAMES
    through the encoder at both places instead, the reference's data flow (needs a bank that keeps its frames).  ``context_size``: 19
    in the reference.  ``return_intermediates`` adds ``first_pass_codes`` [B,S,t,t], ``first_pass_camera`` [B,7], ``nearest``
    [B,num_gen_ctx], ``context_indices`` [B,context_size] and the keys of ``evaluate.generate_batch_predictions(return_codes=True)``."""
    if not transformer_model.use_localization:
        raise RuntimeError('pose refinement needs a model with the localization head')
    dev = codebook_model.device
    B = torch.as_tensor(cameras).shape[0]
    n_fill = context_size - num_gen_ctx
    if not 0 <= num_gen_ctx <= context_size:
        raise ValueError(f'num_gen_ctx {num_gen_ctx}: 0 .. context_size = {context_size} expected')
    if fill_indices is None:
        fill_indices = [draw_fill_indices(bank, n_fill, rng) for _ in range(B)]
    fill = torch.as_tensor(fill_indices, dtype=torch.int32).reshape(B, n_fill).to(dev)
    images = torch.as_tensor(images).to(dev)
    cameras = torch.as_tensor(cameras, dtype=torch.float32).to(dev)
    gt_cameras, gt_frames = cameras[:, -1], images[:, -1]                                     # :158
    transform = None
    if transformer_model.config.augment_poses == 'relative':                                  # :160-162
        cameras, transform = geometry.to_relative_cameras(cameras)
    cameras = geometry.normalize_cameras(cameras)                                             # :163
    codes = _view_codes(bank, transformer_model, codebook_model, images, context_indices, reencode)   # :165-177
    generated_cameras, _ = _localize(transformer_model, codes, cameras)                       # :180-181
    if transform is not None:                                                                 # :184-185
        generated_cameras = geometry.from_relative_cameras(generated_cameras, transform)
    first = generated_cameras[:, 0, :].contiguous()
    # :188-189 (num_gen_ctx = 0, main's default: an all-random context)
    nearest = bank.nearest(first, num_gen_ctx) if num_gen_ctx else torch.empty((B, 0), dtype=torch.int32, device=dev)
    ctx_idx = torch.cat((nearest, fill), 1)                                                   # :190-191
    if reencode:
        ctx_cameras = bank.gather(ctx_idx)[1]
        frames = torch.cat((bank.frames_at(ctx_idx), gt_frames[:, None]), 1)                  # :196
        new_codes = None
    else:
        ctx_codes, ctx_cameras = bank.gather(ctx_idx)
        frames = gt_frames[:, None]
        new_codes = torch.cat((ctx_codes, codes[:, -1:]), 1)
    new_cameras = torch.cat((ctx_cameras, gt_cameras[:, None]), 1)                            # :195
    res = evaluate.generate_batch_predictions(transformer_model, codebook_model, frames, new_cameras, return_codes=return_intermediates,
                                              codes=new_codes)                                # :197
    if return_intermediates:
        res.update(first_pass_codes=codes, first_pass_camera=first, nearest=nearest, context_indices=ctx_idx)
    return res


def _generated_images_scene(transformer_model, codebook_model, codes, cameras, transform, num_gen_ctx, uniforms, fused_passes, keep):
    """:102-148 for ONE scene (B = 1 tensors, as the reference's ``expand_dims(new_codes, 0)`` requires)"""
    t = transformer_model.config.token_image_size
    nE = transformer_model.config.n_embeddings
    n = num_gen_ctx
    mask = torch.full_like(codes[:, :1], transformer_model.mask_token)
    first_camera, first_pose = _localize(transformer_model, codes, cameras)                   # :103-104
    new_cameras = generate_other_viewpoints(first_camera[:, -1:].repeat(n, 1, 1), uniforms)   # :107
    new_cameras = geometry.normalize_cameras(new_cameras)                                     # :108
    ids2 = torch.cat([codes[:, :-1], mask], 1).repeat(n, 1, 1, 1)                             # :110-113
    poses2 = torch.cat((cameras[:, :-1].repeat(n, 1, 1), new_cameras), 1)                     # :114-117
    out = transformer_model(dict(input_ids=ids2, poses=poses2), training=False, last_view_logits_only=keep, last_view_codes_only=not keep)
    if keep:
        lg2 = out['logits_last']
        new_codes = ops.argmax_rows(lg2.view(-1, nE), n * t * t, nE).view(n, t, t)            # :119 (ties -> lowest index)
    else:
        lg2, new_codes = None, out['codes_last'].view(n, t, t)
    new_codes = new_codes.to(torch.int32)
    codes = torch.cat((codes[:, :-n], new_codes[None]), 1)                                    # :120-123 (sic: the target goes too)
    cameras = torch.cat((cameras[:, :-n], new_cameras.reshape(1, n, -1)), 1)                  # :124-127
    # the final generation pass (:130-134) and the final localization pass (:143-144): the pair MIGT.generate_and_localize fuses
    if fused_passes:
        gen, pose_last = transformer_model.generate_and_localize(codes, cameras, codes_only=not keep)
        lg3 = gen if keep else None
    else:
        out3 = transformer_model(dict(input_ids=torch.cat([codes[:, :-1], mask], 1), poses=cameras), training=False,
                                 last_view_logits_only=keep, last_view_codes_only=not keep)
        lg3 = out3['logits_last'] if keep else None
        gen = lg3 if keep else out3['codes_last']
        pose_last = _localize(transformer_model, codes, cameras)[1]
    generated_codes = ops.argmax_rows(lg3.view(-1, nE), t * t, nE).view(1, t, t) if keep else gen.view(1, t, t)
    dec = codebook_model.decode_code(generated_codes)                                         # :138
    if codebook_model.data_format == 'NCHW':
        dec = dec.permute(0, 2, 3, 1)
    generated_images = ops.postprocess_u8(dec.contiguous())                                   # :139-140
    generated_cameras = transformer_model.reduce_cameras(pose_last, -2)                       # :144
    if transform is not None:                                                                 # :147-148
        generated_cameras = geometry.from_relative_cameras(generated_cameras, transform)
    res = dict(generated_images=generated_images, generated_cameras=generated_cameras[:, -1])
    if keep:
        res.update(first_pass_pose=first_pose, first_pass_camera=first_camera[:, -1], new_cameras=new_cameras[None],
                   pass2_input_ids=ids2[None], pass2_poses=poses2[None], pass2_logits_last=lg2[None], new_codes=new_codes[None],
                   final_codes=codes, final_cameras=cameras, logits_last=lg3, pose_last=pose_last, generated_codes=generated_codes)
    return res


def generate_batch_predictions_using_generated_images(transformer_model, codebook_model, images, cameras, num_gen_ctx: int = 5,
                                                      uniforms=None, seed=0, return_intermediates: bool = False, codes=None,
                                                      fused_passes: bool = True):
    """:80-154, literal for one scene and applied per scene for B > 1: first localization pass, ``num_gen_ctx`` perturbed cameras
    (``generate_other_viewpoints``), one generation pass of batch ``num_gen_ctx``, the last ``num_gen_ctx`` views — the target among
    them (sic) — replaced by the generated code maps and cameras, final generation pass, decode, final localization pass.
    ``uniforms`` [num_gen_ctx,1,8] (every scene) or [B,num_gen_ctx,1,8]; default: the counter hash of ``seed`` (an int for every scene,
    or B ints), so a scene's result does not depend on its batch-mates.  ``codes`` [B,S,t,t]: the views' codes when the caller has them
    (``images`` is then read for ``ground_truth_images`` only).  ``fused_passes=False``: the last two transformer passes as the
    reference's two separate calls (bit-identical).  ``return_intermediates`` adds every transformer pass's inputs and outputs
    (``codes``, ``cameras``, ``first_pass_pose``, ``first_pass_camera``, ``new_cameras``, ``pass2_*``, ``new_codes``, ``final_codes``,
    ``final_cameras``, ``logits_last``, ``pose_last``, ``generated_codes``)."""
    if not transformer_model.use_localization:
        raise RuntimeError('generated_images needs a model with the localization head')
    dev = codebook_model.device
    images = torch.as_tensor(images).to(dev)
    cameras = torch.as_tensor(cameras, dtype=torch.float32).to(dev)
    B, S = cameras.shape[:2]
    if not 1 <= num_gen_ctx <= S:
        raise ValueError(f'num_gen_ctx {num_gen_ctx}: 1 .. {S} views can be replaced')
    ground_truth_cameras = cameras[:, -1]                                                     # :81
    transform = None
    if transformer_model.config.augment_poses == 'relative':                                  # :83-85
        cameras, transform = geometry.to_relative_cameras(cameras)
    cameras = geometry.normalize_cameras(cameras)                                             # :86
    t = transformer_model.config.token_image_size
    if codes is None:
        codes = _encode(codebook_model, transformer_model, images)                            # :88-100
    codes = torch.as_tensor(codes).to(dev).to(torch.int32).view(B, S, t, t)
    seeds = [int(seed)] * B if np.ndim(seed) == 0 else [int(s) for s in seed]
    if uniforms is not None:
        uniforms = torch.as_tensor(uniforms)
    parts = []
    for b in range(B):
        if uniforms is None:
            u = default_uniforms((num_gen_ctx, 1), seeds[b])
        else:
            u = uniforms[b] if uniforms.dim() == 4 else uniforms
        parts.append(_generated_images_scene(transformer_model, codebook_model, codes[b:b + 1], cameras[b:b + 1],
                                             None if transform is None else transform[b:b + 1], num_gen_ctx, u, fused_passes,
                                             return_intermediates))
    res = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    res.update(ground_truth_images=images[:, -1], ground_truth_cameras=ground_truth_cameras)  # :150-154
    if return_intermediates:
        res.update(codes=codes, cameras=cameras)
    return res


def _batched(items, n):
    batch = []
    for it in items:
        batch.append(it)
        if len(batch) == n:
            yield batch
            batch = []
    if batch:
        yield batch


def evaluate_scene(bank, transformer_model, codebook_model, queries, generation_procedure: str = 'standard', num_gen_ctx: int = 0,
                   batch_size: int = 1, match_map=None, top_n_matched_images: int = 0, context_size: int = CONTEXT_SIZE, rng=None,
                   seed: int = 0, lpips=None, store_predictions=None):
    """The per-scene loop of main (:246-279): ``queries`` yields ``(frames uint8 [1,H,W,3], cameras [1,7], file)`` items (the test
    loader's sequences of one view, :248-252, in the order the caller wants them evaluated); every query gets ``context_size`` bank
    views (``build_batch``: its matched files first when ``match_map`` is given) and goes through ``generation_procedure``
    ('standard' | 'generated_images' | 'pose_refinement'), ``batch_size`` queries per call (the reference's loop is batch 1), context
    codes from the bank.  All host draws (context, refinement fill) are made per query in the reference's order, so the predictions do
    not depend on ``batch_size``.  ``rng``: a ``random.Random`` (default ``random.Random(seed)``); ``seed`` + the query's position also
    seeds ``generated_images``' perturbations.  ``store_predictions``: called with every batch's prediction dict, as main does (:269).
    -> ``metrics.Evaluator(image_size=128).result()``."""
    if generation_procedure not in ('standard', 'generated_images', 'pose_refinement'):
        raise ValueError(f'unknown generation_procedure {generation_procedure!r}')
    if top_n_matched_images > 0 and match_map is None:                                        # :217-218
        raise ValueError('top_n_matched_images needs a match_map')
    rng = rng or _random.Random(seed)
    evaluator = metrics.Evaluator(image_size=128, lpips=lpips)                                # :247
    position = 0
    for batch in _batched(queries, batch_size):
        cams, frames, indices, fills = [], [], [], []
        for gt_frames, gt_cameras, file in batch:
            matches = match_map.get(file + '.color.png', [])[:top_n_matched_images] if match_map is not None else ()   # :238-239
            c, _, idx = build_batch(bank, gt_frames, gt_cameras, matches, context_size, rng, context_frames=False)
            cams.append(c)
            frames.append(torch.as_tensor(gt_frames)[None])
            indices.append(idx)
            if generation_procedure == 'pose_refinement':
                fills.append(draw_fill_indices(bank, context_size - num_gen_ctx, rng))        # :191
        cams, frames = torch.cat(cams), torch.cat(frames)                                     # [B,S,7], [B,1,H,W,3]
        if generation_procedure == 'pose_refinement':                                         # :265-267
            pred = generate_batch_predictions_using_pose_refinement(bank, transformer_model, codebook_model, frames, cams,
                                                                    num_gen_ctx=num_gen_ctx, fill_indices=fills,
                                                                    context_size=context_size, context_indices=indices)
        else:
            dev = codebook_model.device
            codes = _view_codes(bank, transformer_model, codebook_model, frames.to(dev), indices, False)
            if generation_procedure == 'standard':                                            # :261-262
                pred = evaluate.generate_batch_predictions(transformer_model, codebook_model, frames, cams, codes=codes)
            else:                                                                             # :263-264
                pred = generate_batch_predictions_using_generated_images(transformer_model, codebook_model, frames, cams,
                                                                         num_gen_ctx=num_gen_ctx, codes=codes,
                                                                         seed=[seed + position + i for i in range(len(batch))])
        position += len(batch)
        evaluator.update_state(**pred)                                                        # :268
        if store_predictions is not None:
            store_predictions(**pred)
    return evaluator.result()                                                                 # :272


def evaluate_scene_multictx(bank, transformer_model, codebook_model, queries, batch_size: int = 1, context_size: int = CONTEXT_SIZE,
                            rng=None, seed: int = 0, lpips=None, store_predictions=None):
    """evaluate_sevenscenes_multictx.py:36-63: every query with ``context_size`` random bank views through the multi-context pass
    (``evaluate_multictx.generate_batch_predictions``: the target generated and localized from 0 .. S-1 context views) into a
    ``metrics.MultiContextEvaluator(context_size + 1, image_size=128)``.  That pass takes frames: the bank must keep its pixels."""
    rng = rng or _random.Random(seed)
    evaluator = metrics.MultiContextEvaluator(context_size + 1, image_size=128, lpips=lpips)  # :46
    for batch in _batched(queries, batch_size):
        built = [build_batch(bank, f, c, (), context_size, rng) for f, c, _ in batch]         # :36-43
        if built[0][1].shape[1] != context_size + 1:
            raise RuntimeError('evaluate_scene_multictx needs a SceneBank that keeps its frames')
        pred = evaluate_multictx.generate_batch_predictions(transformer_model, codebook_model, torch.cat([b[1] for b in built]),
                                                            torch.cat([b[0] for b in built]))  # :56
        evaluator.update_state(**pred)                                                        # :57
        if store_predictions is not None:
            store_predictions(**pred)
    return evaluator.result()
