"""Many query views from ONE context: novel-view rendering without target frames, and localization of photos.

``evaluate.generate_batch_predictions`` is the evaluator's loop body: S views in, one view out, and it wants an image for the view it is
about to generate.  An orbit of N views around C photographs costs it N * (C + 1) encoder passes and N * (C + 1) transformer views.  The
model allows the saving exactly: the context views never see the target, so their encoder codes and every layer's keys
and values are computed once (``MIGT.prefill_context``) and each query is a single MASK view attending to that cache
(``MIGT.generate_from_context`` -> ``ops.attn_prefix``): C encodes, C context views, N query views, N decodes.

    r = ViewRenderer(transformer_model, codebook_model)
    r.set_context(images=frames_u8, cameras=cams)            # or codes=... (scene_bank.SceneBank.gather)
    out = r.render(query_cameras)                            # out['generated_images'] uint8 [B,N,H,W,3]
    swp = r.sweep(query_cameras)                             # swp['generated_images'] uint8 [B,N,C+1,H,W,3]: the view from 0, 1, ..., C photos
    est = r.localize(images=photos_u8)                       # est['generated_cameras'] fp32 [B,N,7], the caller's world frame
    fit = r.score(candidate_cameras, images=photo_u8)        # fit['log_likelihood'] fp32 [B,N]: how well the photo fits each camera
    alt = r.sample(query_cameras, n_samples=8, top_p=0.9)    # alt['generated_images'] uint8 [B,N,8,H,W,3]: draws, with their log-likelihood
    avg = r.render_mean(query_cameras, top_p=0.9)            # avg['generated_images'] uint8 [B,N,H,W,3]: the mean of those draws' latents, decoded once
    r.append(images=new_frames_u8, cameras=new_cams)         # new photographs: the context grows by K views, no earlier view is run again
    fly = r.rollout(path_cameras)                            # fly['generated_images'] uint8 [B,T,H,W,3]: frame t sees the photos AND frames 0..t-1

Contract: ``render(q)['generated_images'][b, n]`` is what ``generate_batch_predictions`` generates for the scene (context views of b...,
any frame) with cameras (context cameras of b..., q[b, n]); ``localize(photos)['generated_cameras'][b, n]`` is what it returns as
``generated_cameras`` for the scene (context views of b..., photos[b, n]) with cameras (context cameras of b..., anything).

Localization uses the same cache: the LOC view of a photo is ``wte[codes] + wpe + wte[LOC]`` — no pose — and sees the
context and itself, so N photos against C context photographs cost N encodes and N transformer views
(``MIGT.localize_from_context``) instead of N * (C + 1) of each; one ``set_context`` serves ``render`` and ``localize`` alike.

Context lengths: the context is block-causal, ``wpe`` indexes the token inside a view and the cameras are relative to
view 0 camera by camera, so the first c views of a C-view cache ARE the cache of those c views.  ``n_context`` — per scene in
``set_context`` (a ragged batch padded to C), per scene or per query view in the four methods — makes a query walk only that many prefix
tiles (``ops.attn_prefix(ctx_len=...)``): ``sweep`` answers "how good is the view from 0, 1, ..., C photos" from one prefill, and
``evaluate_context_sizes`` is the cached drop-in for ``evaluate_multictx.generate_batch_predictions``.

A context that grows: for the same three reasons a view added BEHIND the cached ones changes none of them.  A cache
with room (``set_context(capacity=...)``; otherwise it is reallocated, doubling) takes the keys and values of new views in every layer
(``ops.kv_append``), and a new view attends to the cache, the new views before it and itself through the same prefix attention:
``append`` costs the K new views and nothing else, and ``rollout`` generates a camera path autoregressively — frame t from the photographs
and the frames 0 ... t-1 — in one two-view pass per step, codes fed back on the device.  Contract: ``append(x, cams)`` after
``set_context(ctx, ctx_cams)`` answers every later call as ``set_context(cat(ctx, x), cat(ctx_cams, cams))`` would, within the arm's own
error (the same launches per row, except that a prefilled view's attention is the block-causal kernel and an appended view's the prefix
kernel); ``rollout(path)`` is the loop
"``sample`` one view at path[t] (``top_k = 1``: ``render``), ``append`` it with path[t]".

Forks: S trajectories from one context need not copy it.  ``r.fork(S)`` is a renderer of B*S what-if scenes whose cache
(``ContextCache.fork``) reads r's views where they lie and owns only what it adds; ``r.rollout(path, n_samples=S, fork=True)`` rolls the
trajectories out on such a fork — the bits of the replicated roll-out — and ``adopt='best'`` (or an index per scene) keeps one of them in
r's own context without running a row again.  ``score_gradient`` and ``refine`` need ``cache.materialize()``, the plain copy.

Not covered here: contexts that change per query other than by growing at the end (the 7-Scenes pose-refinement loop; sliding windows or
eviction, which would change what the later views' keys are); they keep their evaluator.
"""
import numpy as np
import torch

from . import geometry
from . import ops
from .evaluate import MAX_SCENES_PER_CALL, _frames_for_encode


def context_poses(context_cameras, augment_poses: str):
    """The context's model poses and the transform that made them: cameras [B,C,7] in the caller's world frame ->
    (poses [B,C,7], transform [B,1,7] or None) — ``to_relative_cameras`` (relative to view 0) when the model was trained with
    ``augment_poses == 'relative'``, then ``normalize_cameras``: evaluate_transformer.py:99-102."""
    transform = None
    if augment_poses == 'relative':
        context_cameras, transform = geometry.to_relative_cameras(context_cameras)
    return geometry.normalize_cameras(context_cameras), transform


def query_poses(query_cameras, transform):
    """Query cameras [B,N,7] in the caller's world frame -> model poses [B,N,7] in the context's frame.  ``transform``: view 0's camera
    [B,1,7] from ``context_poses`` (None: no relativisation).  Equal, bit for bit, to the last camera of
    ``normalize_cameras(to_relative_cameras(cat(context, query_n)))`` for every n: both relativise with view 0's camera, camera by
    camera (tests/test_render_host.py)."""
    if transform is not None:
        # to_relative_cameras reads its transform from the first camera of the sequence: put view 0 in front, drop it afterwards
        query_cameras = geometry.to_relative_cameras(torch.cat([transform, query_cameras], -2))[0][..., 1:, :]
    return geometry.normalize_cameras(query_cameras)


def ascend_poses(poses, grad, step_xyz, step_rot):
    """One ascent step on model poses [...,7] (position, unit quaternion) along a gradient [...,7] w.r.t. the 7 numbers taken as free:
    position + step_xyz * g_xyz / ||g_xyz||; quaternion + step_rot * t / ||t|| with t the part of g_q tangent to the unit sphere at q
    (g_q - (g_q . q) q: the radial part changes nothing, the model input is read after normalisation by every caller), then
    renormalised and sign-removed as ``normalize_cameras`` does.  A zero (or non-finite) block does not move, nor does a quaternion whose
    gradient is radial (tangent part below 1e-6 of it).  ``step_*``: a number or a
    tensor broadcastable to ``poses[..., 0]``.  Pure torch on [...,7] tensors: no model, no launch of the library."""
    poses = torch.as_tensor(poses, dtype=torch.float32)
    grad = torch.as_tensor(grad, dtype=torch.float32).to(poses.device)
    if poses.shape != grad.shape or poses.shape[-1] != 7:
        raise ValueError(f'ascend_poses: poses and grad [...,7] of one shape expected, got {tuple(poses.shape)} and {tuple(grad.shape)}')

    def step(x):                                                     # a number fills a tensor on the device (no copy from the host)
        if isinstance(x, torch.Tensor):
            return x.to(device=poses.device, dtype=torch.float32).expand(poses.shape[:-1]).unsqueeze(-1)
        return torch.full((*poses.shape[:-1], 1), float(x), dtype=torch.float32, device=poses.device)

    sx, sr = step(step_xyz), step(step_rot)

    def unit(v, floor=0.0):
        n = v.norm(dim=-1, keepdim=True)
        ok = torch.isfinite(n) & (n > floor)
        return torch.where(ok, v / torch.where(ok, n, torch.ones_like(n)), torch.zeros_like(v))

    q = geometry.quaternion_normalize(poses[..., 3:])
    gq = grad[..., 3:]
    tangent = gq - (gq * q).sum(-1, keepdim=True) * q
    xyz = poses[..., :3] + sx * unit(grad[..., :3])
    ut = unit(tangent, floor=1e-6 * gq.norm(dim=-1, keepdim=True))       # a purely radial g_q leaves rounding noise, not a direction
    moved = (ut != 0).any(-1, keepdim=True)
    quat = geometry.quaternion_remove_sign(geometry.quaternion_normalize(q + sr * ut))
    return torch.cat((xyz, torch.where(moved, quat, poses[..., 3:])), -1)


def default_views_per_call(n_scenes: int) -> int:
    """Query views per scene in one transformer pass: at most MAX_SCENES_PER_CALL view-rows over the batch, the evaluator's own cap
    (one query view has the activations of one of its scenes' views; the cap keeps every activation below 32-bit offsets)."""
    return max(1, MAX_SCENES_PER_CALL // max(1, n_scenes))


def plan_view_chunks(n_views: int, n_scenes: int = 1, max_views_per_call: int = None):
    """[(start, stop)) ranges over the N query views of every scene: whole views, in order, each view exactly once, at most
    ``max_views_per_call`` (default ``default_views_per_call(n_scenes)``) per range; [] for N = 0.  Pure: no device, no model."""
    cap = default_views_per_call(n_scenes) if max_views_per_call is None else int(max_views_per_call)
    if cap < 1 or n_views < 0:
        raise ValueError(f'plan_view_chunks: max_views_per_call >= 1 and n_views >= 0 expected, got {cap} and {n_views}')
    return [(a, min(a + cap, n_views)) for a in range(0, n_views, cap)]


def _int_array(what, x, ndim=(1,), low: int = 0):
    """``x`` — host data or a tensor (a device tensor is brought to the host once) — as a numpy array of integers, not bool, with one
    of ``ndim`` dimensions and no value below ``low``; anything else: ValueError naming ``what``.  Pure."""
    a = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x)
    if a.ndim not in ndim or a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer) or (a.size and a.min() < low):
        raise ValueError(f'{what}: integers >= {low} with {" or ".join(map(str, ndim))} dimension(s) expected, got {x}')
    return a


def plan_context_lengths(n_context, B: int, N: int, C: int, scene_default=None):
    """Context lengths of N query views per scene, normalised: ``n_context`` — an int, [B] (one length per scene) or [B,N] (one per
    query view) of integers in [0, C]; host data preferred, a device tensor is brought to the host once — -> int32 array [B,N].
    ``None`` -> ``scene_default`` ([B], e.g. ``set_context``'s) broadcast the same way, or None without one (today's rectangular path).
    Floats, bools, values outside [0, C] and other shapes raise ValueError.  Pure: no device, no model."""
    if n_context is None:
        n_context = scene_default
        if n_context is None:
            return None
    if isinstance(n_context, torch.Tensor):
        n_context = n_context.detach().cpu().numpy()
    a = np.asarray(n_context)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f'n_context: integers expected, got {a.dtype}')
    if a.ndim == 0:
        a = np.broadcast_to(a, (B, N))
    elif a.shape == (B,):
        a = np.broadcast_to(a.reshape(B, 1), (B, N))
    elif a.shape != (B, N) or a.ndim != 2:
        raise ValueError(f'n_context: an int, [B={B}] or [B={B},N={N}] expected, got {a.shape}')
    if a.size and (a.min() < 0 or a.max() > C):
        raise ValueError(f'n_context: values in [0, C={C}] expected, got {int(a.min())} ... {int(a.max())}')
    return np.array(a, dtype=np.int32, order='C')                  # always a copy: the caller's array (or a broadcast view) stays as it is


def sweep_layout(N: int, K: int):
    """The order in which ``ViewRenderer.sweep`` renders N cameras at K context sizes, and the way back: (camera [K*N], size [K*N],
    inverse [N,K]).  Rendered view j is camera ``camera[j]`` at size number ``size[j]``, SIZE-MAJOR (j = k N + n): consecutive views
    have equal lengths, so the attention's groups of 4 / 2 consecutive views stay homogeneous.  ``inverse[n, k]`` = the rendered index
    of (camera n, size k): ``x[:, inverse.reshape(-1)].view(B, N, K, ...)`` is the result per camera.  Pure."""
    if N < 0 or K < 0:
        raise ValueError(f'sweep_layout: N >= 0 and K >= 0 expected, got {N} and {K}')
    j = np.arange(K * N, dtype=np.int64)
    inverse = (np.arange(K, dtype=np.int64).reshape(1, K) * N + np.arange(N, dtype=np.int64).reshape(N, 1))
    return (j % N if N else j), (j // N if N else j), inverse


def plan_capacity(capacity: int, needed: int) -> int:
    """The capacity (views per scene) of a cache that must hold ``needed`` views: ``capacity`` while it suffices, else
    max(2 capacity, needed) — doubling, so that T appends of one view reallocate O(log T) times.  Pure."""
    capacity, needed = int(capacity), int(needed)
    if capacity < 0 or needed < 0:
        raise ValueError(f'plan_capacity: capacity >= 0 and needed >= 0 expected, got {capacity} and {needed}')
    return capacity if needed <= capacity else max(2 * capacity, needed)


def plan_cache_bytes(B: int, C: int, L: int, d_model: int, n_head: int, n_layer: int, elem_bytes: int, form=None) -> int:
    """The bytes of a context cache of B scenes x C views of room, from its shapes (``ContextCache.nbytes``): ``form`` None = the plain
    cache ([B*C*L, 3 d] per layer), 'kv' = the K/V-only pack ([B*C*L, d] twice: exactly 2/3), 'e4m3' = the e4m3 pack (two byte tiles
    [B*C, H, 64, 64] and two fp32 scales [B*C, H] per layer; ``elem_bytes`` does not enter).  A GROWING packed cache
    (``pack(room=...)``) holds the same tensors with C = its ``capacity``: pass that.  Pure."""
    B, C, L, d, H, n = int(B), int(C), int(L), int(d_model), int(n_head), int(n_layer)
    if min(B, C, L, d, H, n) < 0 or int(elem_bytes) not in (2, 4):
        raise ValueError(f'plan_cache_bytes: sizes >= 0 and elem_bytes 2 or 4 expected, got {(B, C, L, d, H, n, elem_bytes)}')
    if form is None:
        return n * B * C * L * 3 * d * int(elem_bytes)
    if form == 'kv':
        return n * 2 * B * C * L * d * int(elem_bytes)
    if form == 'e4m3':
        return n * 2 * (B * C * H * 64 * 64 + B * C * H * 4)
    raise ValueError(f"plan_cache_bytes: form None, 'kv' or 'e4m3' expected, got {form!r}")


def plan_rollout_lengths(lengths, T: int):
    """Context lengths of a T-step roll-out from scenes of ``lengths`` [B] filled views: (gen int32 [T,B], pair int32 [T,B,2]).
    ``gen[t, b] = lengths[b] + t``: what the MASK view of step t sees (the context and the generated views 0 ... t-1), and also the
    cache view that the generated view t is appended at, seeing as many.  ``pair[t, b]`` = (gen[t-1, b], gen[t, b]): the fused step's
    two views per scene, the append view of step t-1 and the MASK view of step t (row 0, which has no append view, is not used).  Pure."""
    a = _int_array('plan_rollout_lengths: lengths [B]', lengths)
    if T < 0:
        raise ValueError(f'plan_rollout_lengths: T >= 0 expected, got {T}')
    gen = (a.astype(np.int64).reshape(1, -1) + np.arange(T, dtype=np.int64).reshape(T, 1)).astype(np.int32)
    pair = np.stack([gen - 1, gen], -1)
    return np.ascontiguousarray(gen), np.ascontiguousarray(pair)


def plan_replication(B: int, S: int):
    """Scene of the original batch behind each scene of a batch replicated S times: int64 [B*S], scene b's copies at b*S ... b*S+S-1.  Pure."""
    if B < 0 or S < 1:
        raise ValueError(f'plan_replication: B >= 0 and S >= 1 expected, got {B} and {S}')
    return np.repeat(np.arange(B, dtype=np.int64), S)


def plan_fork(lengths, S: int):
    """The children of a fork of scenes with ``lengths`` [B] filled views, S per scene: (split int32 [B*S], parent int64 [B*S]).  Child
    scene b*S+s (the order of ``plan_replication``) starts at ``split = lengths[b]`` logical views, all of them parent scene b's.  Pure."""
    a = _int_array('plan_fork: lengths [B]', lengths)
    if S < 1:
        raise ValueError(f'plan_fork: S >= 1 expected, got {S}')
    parent = plan_replication(a.shape[0], S)
    return np.ascontiguousarray(a[parent].astype(np.int32)), parent


def map_fork_views(split, n_views: int):
    """Where the logical views 0 ... n_views-1 of every scene of a fork lie: (segment int8 [B,n_views], view int32 [B,n_views]) —
    segment 0 = the parent's buffers, view s, for s < split[b]; segment 1 = the scene's own buffers, view s - split[b], otherwise.  This
    is the mapping of ``vf_attn_prefix_fork_*`` and of the own-buffer appends.  Pure."""
    a = _int_array('map_fork_views: split [B]', split)
    if n_views < 0:
        raise ValueError(f'map_fork_views: n_views >= 0 expected, got {n_views}')
    s = np.arange(n_views, dtype=np.int64).reshape(1, n_views)
    sp = a.astype(np.int64).reshape(-1, 1)
    own = s >= sp
    return own.astype(np.int8), np.where(own, s - sp, s).astype(np.int32)


def plan_fork_lengths(split, lengths, room: int):
    """The own views of a fork's scenes: ``lengths - split`` int32 [B], validated — logical ``lengths`` [B] of at least ``split`` and at
    most ``split + room``, and the same number of own views in every scene (children grow together).  Pure."""
    sp, ln = _int_array('plan_fork_lengths: split [B]', split), _int_array('plan_fork_lengths: lengths [B]', lengths)
    if sp.shape != ln.shape or room < 0 or (ln < sp).any() or (ln > sp.astype(np.int64) + room).any():
        raise ValueError(f'plan_fork_lengths: split <= lengths <= split + room = {room}, [B] integers, expected, got {split} and {lengths}')
    own = (ln.astype(np.int64) - sp).astype(np.int32)
    if own.size and (own != own[0]).any():
        raise ValueError(f'plan_fork_lengths: every scene holds the same number of own views, got {own.tolist()}')
    return own


def choose_best(score):
    """The trajectory to keep per scene: ``score`` [B,S] floats -> int64 [B], the index of the largest score, ties going to the lowest
    index; a NaN never wins against a number (a row of NaNs gives 0).  Pure."""
    a = np.asarray(score, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError(f'choose_best: score [B,S >= 1] expected, got {a.shape}')
    return np.argmax(np.where(np.isnan(a), -np.inf, a), axis=1).astype(np.int64)


def rollout_row_ids(n_scenes: int, t: int, L: int):
    """Noise keys of step t of a roll-out over ``n_scenes`` (= B*S) scenes: int64 [n_scenes*L], (scene << 32) | (t L + l) — what
    ``MIGT.sample_from_context`` gives view ``t`` of that scene (``view0 = t``), so a trajectory's draws do not depend on T.  Pure."""
    if n_scenes < 0 or t < 0 or L < 1 or (t + 1) * L > 1 << 32:
        raise ValueError(f'rollout_row_ids: n_scenes >= 0, t >= 0, L >= 1 and (t + 1) L <= 2^32 expected, got {n_scenes}, {t}, {L}')
    return ((np.arange(n_scenes, dtype=np.int64) << 32).reshape(-1, 1) + (np.arange(L, dtype=np.int64) + t * L).reshape(1, L)).reshape(-1)


class ViewRenderer:
    def __init__(self, transformer_model, codebook_model):
        self.transformer = transformer_model
        self.codebook = codebook_model
        self.cache = None
        self.transform = None
        self.context_codes = None
        self.n_context = None              # set_context(n_context=...): valid context views per scene, int32 [B] (host), the methods' default
        self.fused_score = None            # score: None = MIGT.score_from_context's default route, True / False = the fused LM head / through the logits
        self.fused_tail = None             # localize: None = MIGT.localize_from_context's default tail, True / False = the fused / unfused one

    def set_context(self, images=None, cameras=None, codes=None, n_context=None, capacity=None, pack=None):
        """``images`` uint8 [B,C,H,W,3] (host or device; resized for the encoder as the evaluators do) or ``codes`` int [B,C,t,t]
        (already encoded, e.g. ``SceneBank.gather``), and ``cameras`` [B,C,7] in the caller's world frame.  Encodes once, prefills the
        transformer's key / value cache once.  ``n_context``: [B] (or an int), the number of valid context views per scene in [1, C],
        for a ragged batch padded to C: scene b's queries see its first ``n_context[b]`` views only (the default of ``render``,
        ``sample``, ``score``, ``localize`` and ``sweep``).  Padding views must hold valid code ids (or images) and finite cameras; they
        are computed by the prefill and never read by a query.  View 0 is valid in every scene, so the poses' frame is each scene's own.
        ``capacity`` >= C: room for that many views per scene (``MIGT.prefill_context``), so that ``append`` and ``rollout`` need not
        reallocate; None: the tight cache, which grows at the first of them.
        ``pack``: None, ``'kv'`` or ``'e4m3'`` (bf16 models): the context is filled as a GROWING packed cache of that form directly
        (``MIGT.prefill_context(pack=...)``: the plain cache never exists), as ``set_context(...)`` then ``pack(dtype, room=capacity - C)``
        would leave it, bit for bit."""
        if cameras is None:
            raise ValueError('set_context: cameras expected')
        cameras = self._world_cameras('set_context', cameras, new=True)
        B, C = cameras.shape[:2]
        if C < 1:
            raise ValueError(f'set_context: at least one context view expected, got cameras {tuple(cameras.shape)}')
        if n_context is not None:                                        # an int or [B], in [1, C]: a scene has at least one context view
            n_context = plan_context_lengths(_int_array('set_context: n_context', n_context, ndim=(0, 1), low=1), B, 1, C)[:, 0].copy()
        codes = self._photo_codes('set_context', images, codes, B, (C,))
        poses, transform = context_poses(cameras, self.transformer.config.augment_poses)
        kw = {} if pack is None else dict(pack=pack)
        if capacity is not None:
            kw['capacity'] = capacity
        self.cache = self.transformer.prefill_context(codes, poses, **kw)
        self.transform, self.context_codes, self.n_context = transform, codes, n_context
        return self

    def pack(self, dtype=None, room=None):
        """Pack the context in place (``ContextCache.pack``; the plain cache is released) and return ``self``: ``dtype=None`` keeps the
        K and V thirds as they are (2/3 of the bytes, both arms, every answer keeps its bits), ``dtype='e4m3'`` (bf16 models) stores
        them as e4m3 bytes with a power-of-two scale per (scene, view, head) — about 1/3 of the bf16 bytes, the answers of the bf16 arm
        on the dequantised cache.  ``render``, ``sample``, ``score``, ``localize`` and ``sweep`` go on working; ``append``, ``rollout``,
        ``fork``, ``score_gradient`` and ``refine`` refuse until ``unpack()``.  ``room=R`` (an integer >= 0; opt-in): the GROWING packed
        form with R views of slack per scene (``ContextCache.pack(room=...)``), on which ``append`` and ``rollout`` (``keep``,
        ``n_samples``; not ``fork=True``) go on working; ``fork``, ``score_gradient`` and ``refine`` still refuse until ``unpack()``."""
        self._context('pack')
        self.cache = self.cache.pack(dtype) if room is None else self.cache.pack(dtype, room=room)
        return self

    def unpack(self):
        """Undo ``pack``: a plain cache again (the K/V-only form bit for bit, the e4m3 form dequantised; the Q third zeros), in place."""
        self._context('unpack')
        self.cache = self.cache.unpack()
        return self

    def context_bytes(self):
        """the bytes of the context cache's own tensors, from their shapes"""
        self._context('context_bytes')
        return self.cache.nbytes()

    def _context(self, what):
        """the context cache, for ``what``"""
        if self.cache is None:
            raise RuntimeError(f'ViewRenderer.{what}: set_context() first')
        return self.cache

    def _refuse_packed(self, what):
        self.cache.refuse_packed(f'ViewRenderer.{what}')

    def _refuse_growth(self, what):
        self.cache.refuse_growth(f'ViewRenderer.{what}')

    def _own_lengths(self, cache):
        """before the context grows: a ragged batch's valid views (``set_context(n_context=...)``) become the cache's own lengths, so
        that new views go behind each scene's valid views (over its padding)"""
        if self.n_context is not None and cache.lengths is None:
            cache.lengths = np.array(self.n_context, dtype=np.int32)
            cache.C = int(cache.lengths.max())
        return cache

    def _add_codes(self, before, codes):
        """context_codes [B,C,t,t] with ``codes`` [B,K,t,t] behind each scene's ``before[b]`` valid maps (padded to the longest scene)"""
        B, K = codes.shape[:2]
        old = self.context_codes
        C = int(before.max()) + K
        out = torch.zeros((B, max(C, old.shape[1]), *old.shape[2:]), dtype=old.dtype, device=old.device)
        out[:, :old.shape[1]] = old
        at = torch.from_numpy(before.astype(np.int64).reshape(B, 1) + np.arange(K, dtype=np.int64).reshape(1, K)).to(old.device)
        out[torch.arange(B, device=old.device).view(B, 1), at] = codes.to(old.dtype)
        self.context_codes = out[:, :C]
        if self.n_context is not None:
            self.n_context = (before + K).astype(np.int32)

    def append(self, images=None, codes=None, cameras=None):
        """New photographs arrive: ``images`` uint8 [B,K,H,W,3] (encoded once, as ``set_context`` encodes) or ``codes`` int [B,K,t,t], and
        ``cameras`` [B,K,7] in the caller's world frame (the context's: view 0 stays the frame).  The context grows in place by K views
        per scene in one pass over the new views (``MIGT.append_to_context``): no earlier view is run again.  Every later ``render``,
        ``sample``, ``score``, ``localize`` and ``sweep`` sees the grown context; ``n_context`` and ``context_codes`` follow."""
        self._context('append')
        self._refuse_growth('append')
        if cameras is None:
            raise ValueError('append: cameras expected')
        cameras = self._world_cameras('append', cameras)
        codes = self._photo_codes('append', images, codes, self.cache.B, (cameras.shape[1],))
        self._own_lengths(self.cache)
        before = self.cache.filled()
        self.transformer.append_to_context(self.cache, codes, query_poses(cameras, self.transform))
        self._add_codes(before, codes)
        return self

    def fork(self, S: int, room=None):
        """S what-if renderers per scene: a new ViewRenderer of B*S scenes (scene b's children at b*S ... b*S+S-1) on the same model
        objects, whose cache is ``self.cache.fork(S, room)`` — it reads this renderer's context where it lies and owns only what it
        adds — with ``transform``, ``context_codes`` and ``n_context`` repeated per child.  Its ``append``, ``rollout(keep=True)``,
        ``render``, ``sample``, ``score`` and ``localize`` work as on any renderer and never touch this one; ``score_gradient`` and
        ``refine`` need ``cache.materialize()``."""
        self._context('fork')
        self._refuse_packed('fork')
        if isinstance(S, bool) or int(S) != S or int(S) < 1:
            raise ValueError(f'fork: S, an integer >= 1, expected, got {S}')
        S = int(S)
        r = ViewRenderer(self.transformer, self.codebook)
        r.fused_score, r.fused_tail = self.fused_score, self.fused_tail
        work = self._own_lengths(self.cache.alias())                         # (the ragged batch's valid views: the children start behind them)
        r.cache = work.fork(S, room)
        r.transform = None if self.transform is None else self.transform.repeat_interleave(S, 0)
        r.context_codes = self.context_codes.repeat_interleave(S, 0)
        r.n_context = None if self.n_context is None else np.repeat(self.n_context, S).astype(np.int32)
        return r

    def rollout(self, path_cameras, n_samples: int = 1, temperature: float = 1.0, top_k: int = 1, top_p: float = 1.0, seed: int = 0,
                return_codes: bool = False, keep: bool = True, fused_step: bool = None, fork: bool = False, adopt=None):
        """A fly-through whose frames agree with each other: ``path_cameras`` [B,T,7] in the caller's world frame.  Frame t is generated
        from the photographs AND the frames 0 ... t-1 (``MIGT.rollout_from_context``: the model's autoregressive answer), where
        ``render(path)`` draws every frame from the photographs alone -> dict(generated_images uint8 [B,T,H,W,3], log_likelihood fp32
        [B,T]) — [B,S,T,...] for ``n_samples`` = S > 1, S independent trajectories; with ``return_codes`` also generated_codes int64,
        token_log_prob fp32 [B,(S,)T,t,t] and logits fp32 [B,(S,)T,t,t,n_embeddings].  ``top_k = 1`` (default) is the arg-max roll-out;
        ``temperature``, ``top_k``, ``top_p`` and ``seed`` as ``sample``.  Nothing is decoded inside the loop: the T maps are decoded
        afterwards in chunks of MAX_SCENES_PER_CALL.  ``keep`` (default, S = 1): the generated frames stay in the context, as ``append``
        would leave them; ``keep=False`` rolls out on a copy of the lengths and leaves the renderer's context as it was (the appended
        rows are beyond its lengths again).  With S > 1 the roll-out runs on a replicated cache and the renderer's own is never
        replaced.  ``fused_step``: None = the model's default step, True / False = the one-pass / two-pass step, for A/B runs.
        ``fork=True`` (S > 1; opt-in): the trajectories run on a fork of the context (``MIGT.rollout_from_context(fork=True)``: the
        photographs' keys are shared, not replicated; same bits).  ``adopt`` (with ``fork=True`` and S > 1): ``'best'`` or an int [B] —
        after the roll-out ONE trajectory per scene stays in the renderer's own context (``MIGT.adopt_from_fork``; no row is run
        again), ``'best'`` being the one with the largest sum of ``log_likelihood`` over T, ties going to the lowest index;
        ``context_codes`` and ``n_context`` follow as with ``keep=True`` for S = 1, and the result gains ``adopted`` int64 [B]."""
        self._context('rollout')
        self._refuse_growth('rollout')
        if fork:
            self._refuse_packed('rollout(fork=True)')
        if adopt is not None and not (fork and int(n_samples) > 1):
            raise ValueError('rollout: adopt goes with fork=True and n_samples > 1 (keep=True keeps the one trajectory of n_samples = 1)')
        if adopt is not None and isinstance(adopt, str) and adopt != 'best':
            raise ValueError(f"rollout: adopt 'best' or an int [B] expected, got {adopt!r}")
        tm, B = self.transformer, self.cache.B
        path_cameras = self._world_cameras('rollout', path_cameras)
        S = int(n_samples)
        if S < 1 or S != n_samples:
            raise ValueError(f'rollout: n_samples >= 1 expected, got {n_samples}')
        T = path_cameras.shape[1]
        t = tm.config.token_image_size
        grow = keep and S == 1
        work = self._own_lengths(self.cache if grow or adopt is not None else self.cache.alias())
        before = work.filled()
        kw = {} if fused_step is None else dict(fused_step=bool(fused_step))
        if fork:
            kw['fork'] = True
        out = tm.rollout_from_context(work, query_poses(path_cameras, self.transform), n_samples=S,
                                      temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, return_logits=return_codes, **kw)
        codes = out['codes']                                             # [B,S,T,t,t]
        if grow and T:
            self._add_codes(before, codes[:, 0].to(torch.int32))
        which = None
        if adopt is not None:
            if isinstance(adopt, str):
                which = tm.adopt_from_fork(self.cache, out['cache'], 'best', score=out['log_likelihood'])
            else:
                which = tm.adopt_from_fork(self.cache, out['cache'], adopt)
            if T:
                pick = torch.from_numpy(which).to(codes.device)
                self._add_codes(before, codes[torch.arange(B, device=codes.device), pick].to(torch.int32))
        img, _ = self._decode(codes.reshape(B * S * T, t, t))
        lead = (B, T) if S == 1 else (B, S, T)
        res = dict(generated_images=img.view(*lead, *img.shape[1:]), log_likelihood=out['log_likelihood'].view(*lead))
        if which is not None:
            res['adopted'] = torch.from_numpy(which)
        if return_codes:
            res.update(generated_codes=codes.view(*lead, t, t), token_log_prob=out['token_log_prob'].view(*lead, t, t),
                       logits=out['logits'].view(*lead, t, t, out['logits'].shape[-1]))
        return res

    def _decode(self, flat, keep_decoded: bool = False, latents: bool = False):
        """code maps int [n,t,t] — or, with ``latents``, latent maps fp32 [n,t,t,D] — -> (images uint8 [n,H,W,3], the decoder's fp32
        output [n,H,W,3] or None), decoded in chunks of MAX_SCENES_PER_CALL maps as the evaluators do (``codebook.decode_code``; latents:
        ``codebook.decode``, which takes them in the model's ``data_format``)"""
        cm = self.codebook
        dev = cm.device
        decs, imgs = [], []
        for a in range(0, flat.shape[0], MAX_SCENES_PER_CALL):
            part = flat[a:a + MAX_SCENES_PER_CALL]
            dec = cm.decode(part.permute(0, 3, 1, 2) if cm.data_format == 'NCHW' else part) if latents else cm.decode_code(part)
            if cm.data_format == 'NCHW':
                dec = dec.permute(0, 2, 3, 1)
            dec = dec.contiguous()
            imgs.append(ops.postprocess_u8(dec))
            if keep_decoded:
                decs.append(dec)
        if imgs:
            img = torch.cat(imgs) if len(imgs) > 1 else imgs[0]
        else:
            s = cm.config.image_size
            img = torch.empty((0, s, s, 3), dtype=torch.uint8, device=dev)
        if not keep_decoded:
            return img, None
        dec = torch.cat(decs) if len(decs) > 1 else (decs[0] if decs else torch.empty((0, *img.shape[1:]), dtype=torch.float32, device=dev))
        return img, dec

    def render(self, query_cameras, max_views_per_call: int = None, return_codes: bool = False, return_confidence: bool = False,
               n_context=None):
        """``query_cameras`` [B,N,7] in the caller's world frame (the context's) -> dict(generated_images uint8 [B,N,H,W,3]); with
        ``return_codes`` also generated_codes int64 [B,N,t,t], logits fp32 [B,N,t,t,n_embeddings] and decoded (the decoder's fp32
        output [B,N,H,W,3]).  N is walked in chunks of whole views (``plan_view_chunks``); a view's result does not depend on the
        chunking.  With ``return_confidence`` also confidence and entropy, fp32 [B,N,t,t] each: log p of every generated token and the
        entropy of its distribution (which of a view's tokens the model was guessing), from the LM-head launch that generates the codes.
        ``n_context``: an int, [B] or [B,N] in [0, C] — the number of leading context views each query sees, overriding
        ``set_context``'s per-scene default; sliced per chunk with the views.  4 (bf16) / 2 (f32) consecutive views share an attention
        workgroup, which costs what its longest member costs: keep equal lengths together (``sweep`` does)."""
        self._context('render')
        query_cameras = self._world_cameras('render', query_cameras)
        tm, dev = self.transformer, query_cameras.device
        B, N = self.cache.B, query_cameras.shape[1]
        t = tm.config.token_image_size
        nE = tm.config.n_embeddings
        poses = query_poses(query_cameras, self.transform)
        gen, lgs, conf, ent = [], [], [], []
        for a, b, kw in self._chunks(N, max_views_per_call, n_context):   # (no call at N = 0, unlike ``_walk``: the empties are made here)
            if return_confidence and not return_codes:
                g, cf, en = tm.generate_from_context(self.cache, poses[:, a:b], codes_only=True, return_confidence=True, **kw)
                gen.append(g); conf.append(cf); ent.append(en)
            elif return_codes:
                lg = tm.generate_from_context(self.cache, poses[:, a:b], codes_only=False, **kw)
                lgs.append(lg)
                gen.append(ops.argmax_rows(lg.view(-1, nE), B * (b - a) * t * t, nE).view(B, b - a, t, t))   # ties -> lowest index
                if return_confidence:                      # the logits exist already: the row kernel on them
                    st = ops.logits_score(lg.view(-1, nE), B * (b - a) * t * t, nE, want=('max_logit', 'lse', 'entropy'))
                    conf.append((st['max_logit'] - st['lse']).view(B, b - a, t, t)); ent.append(st['entropy'].view(B, b - a, t, t))
            else:
                gen.append(tm.generate_from_context(self.cache, poses[:, a:b], codes_only=True, **kw))
        codes = torch.cat(gen, 1) if gen else torch.empty((B, 0, t, t), dtype=torch.int64, device=dev)
        img, dec = self._decode(codes.reshape(B * N, t, t), keep_decoded=return_codes)
        res = dict(generated_images=img.view(B, N, *img.shape[1:]))
        if return_codes:
            res.update(generated_codes=codes,
                       logits=torch.cat(lgs, 1) if lgs else torch.empty((B, 0, t, t, nE), dtype=torch.float32, device=dev),
                       decoded=dec.view(B, N, *dec.shape[1:]))
        if return_confidence:
            e = torch.empty((B, 0, t, t), dtype=torch.float32, device=dev)
            res.update(confidence=torch.cat(conf, 1) if conf else e, entropy=torch.cat(ent, 1) if ent else e.clone())
        return res

    def sample(self, query_cameras, n_samples: int = 1, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
               max_views_per_call: int = None, return_codes: bool = False, n_context=None):
        """Draw ``n_samples`` = S plausible views per camera: ``query_cameras`` [B,N,7] in the caller's world frame (the context's) ->
        dict(generated_images uint8 [B,N,S,H,W,3], log_likelihood fp32 [B,N,S]: the log-probability of each drawn code map under the
        distribution it was drawn from); with ``return_codes`` also generated_codes int64 [B,N,S,t,t], token_log_prob fp32 [B,N,S,t,t]
        and kept int32 [B,N,t,t] (the size of the set each token was drawn from).  ``temperature``, ``top_k`` and ``top_p`` trade
        sharpness against diversity (``MIGT.sample_from_context``; ``top_k = 1`` is ``render``).  Draws are reproducible: they depend on
        (seed, the scene's NUMBER b in this context's batch, view number, token, sample number) and not on the batch size, on N or on the
        chunking — N is walked in chunks of whole views (``plan_view_chunks``) and a view's result does not depend on it.  Because the
        noise is keyed by b, a scene set as the context alone (b = 0) and the same scene at b = 1 of a batch get DIFFERENT draws for one
        seed (same distribution, same kept sets, same ``top_k = 1`` result); only scene 0 of a batch reproduces its stand-alone draws.
        ``n_context``: as ``render``'s."""
        self._context('sample')
        query_cameras = self._world_cameras('sample', query_cameras)
        tm = self.transformer
        B, N, S = self.cache.B, query_cameras.shape[1], int(n_samples)
        t = tm.config.token_image_size
        poses = query_poses(query_cameras, self.transform)
        kw = dict(n_samples=S, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
        out = self._walk(N, max_views_per_call, n_context,               # every chunk is told its first view's number (the empty range is not)
                         lambda a, b, **lkw: tm.sample_from_context(self.cache, poses[:, a:b], **(dict(view0=a) if b else {}), **kw, **lkw))
        img, _ = self._decode(out['codes'].reshape(B * N * S, t, t))
        res = dict(generated_images=img.view(B, N, S, *img.shape[1:]), log_likelihood=out['log_likelihood'])
        if return_codes:
            res.update(generated_codes=out['codes'], token_log_prob=out['token_log_prob'], kept=out['kept'])
        return res

    def render_mean(self, query_cameras, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, max_views_per_call: int = None,
                    return_latents: bool = False, n_context=None):
        """The EXPECTED view per camera: ``query_cameras`` [B,N,7] in the caller's world frame (the context's) -> dict(generated_images
        uint8 [B,N,H,W,3], kept int32 [B,N,t,t]: the size of the set each token's mean runs over); with ``return_latents`` also latents
        fp32 [B,N,t,t,D] and decoded (the decoder's fp32 output [B,N,H,W,3]).  A MASK view's tokens are independent given the context,
        so the mean of the distribution ``sample`` draws from (same ``temperature``, ``top_k``, ``top_p``) is known per token in the
        codebook's latent space, q = sum over the kept codes of p_n E[:, n] (``MIGT.expect_from_context``), and costs ONE decode
        (``codebook.decode``, in chunks of MAX_SCENES_PER_CALL views) where averaging S samples costs S.  Where the model is guessing
        the arg-max view commits to one code and the mean view shows the blur; along a camera path it is a continuous function of the
        logits.  ``top_k = 1`` is ``render``, bit for bit, on tokens with a unique maximum.  The codebook must expose
        ``codebook_embedding()``.  N is walked in chunks of whole views (``plan_view_chunks``); a view's result does not depend on the
        chunking.  ``n_context``: as ``render``'s."""
        self._context('render_mean')
        query_cameras = self._world_cameras('render_mean', query_cameras)
        if (not (0 < float(temperature) < float('inf')) or not float(top_p) > 0 or isinstance(top_k, bool) or int(top_k) != top_k
                or int(top_k) < 0):
            raise ValueError(f'render_mean: temperature > 0 (finite), top_p > 0 and an integer top_k >= 0 expected, got {temperature}, '
                             f'{top_p}, {top_k}')
        temperature, top_k, top_p = float(temperature), int(top_k), float(top_p)
        cm, tm = self.codebook, self.transformer
        if not callable(getattr(cm, 'codebook_embedding', None)):
            raise TypeError('render_mean: the codebook model must expose codebook_embedding() (the fp32 [embed_dim, n_embed] device tensor)')
        B, N = self.cache.B, query_cameras.shape[1]
        t = tm.config.token_image_size
        poses = query_poses(query_cameras, self.transform)
        E = cm.codebook_embedding()
        kw = dict(temperature=temperature, top_k=top_k, top_p=top_p)
        out = self._walk(N, max_views_per_call, n_context, lambda a, b, **lkw: tm.expect_from_context(self.cache, poses[:, a:b], E, **kw, **lkw))
        img, dec = self._decode(out['latents'].reshape(B * N, t, t, out['latents'].shape[-1]), keep_decoded=return_latents, latents=True)
        res = dict(generated_images=img.view(B, N, *img.shape[1:]), kept=out['kept'])
        if return_latents:
            res.update(latents=out['latents'], decoded=dec.view(B, N, *dec.shape[1:]))
        return res

    def score(self, query_cameras, images=None, codes=None, max_views_per_call: int = None, n_context=None):
        """How well do photos fit cameras?  ``query_cameras`` [B,N,7] in the caller's world frame (the context's) and ``images`` uint8
        [B,N,H,W,3] or [B,1,H,W,3] (host or device; resized for the encoder as the evaluators do, each photo encoded once) or ``codes``
        int [B,N,t,t] or [B,1,t,t] (already encoded) -> ``MIGT.score_from_context``'s dict: token_log_prob, predicted_codes, confidence,
        entropy [B,N,t,t]; log_likelihood, accuracy [B,N].  One photo per scene (a view axis of 1) is scored against all N cameras:
        ranking candidate poses.  N is walked in chunks of whole views (``plan_view_chunks``); a view's result does not depend on the
        chunking.  ``self.fused_score`` (None = the model's default route, True / False = the fused head / through the logits) is for A/B runs.
        ``n_context``: as ``render``'s."""
        self._context('score')
        query_cameras = self._world_cameras('score', query_cameras)
        N = query_cameras.shape[1]
        photo = self._per_view(self._photo_codes('score', images, codes, self.cache.B, (1, N)), N)
        poses = query_poses(query_cameras, self.transform)
        kw = {} if self.fused_score is None else dict(fused=bool(self.fused_score))
        return self._walk(N, max_views_per_call, n_context,
                          lambda a, b, **lkw: self.transformer.score_from_context(self.cache, poses[:, a:b], photo(a, b), **kw, **lkw))

    # ------------------------------------------------------------------ the front matter, once
    def _world_cameras(self, what, cameras, new: bool = False):
        """``cameras`` [B,N,7] in the caller's world frame (host or device) -> fp32 on the codebook's device; B is the context's, or
        with ``new`` (``set_context``, which has no context yet) the cameras' own"""
        cameras = torch.as_tensor(cameras, dtype=torch.float32).to(self.codebook.device)
        if cameras.dim() != 3 or cameras.shape[-1] != 7 or not (new or cameras.shape[0] == self.cache.B):
            raise ValueError(f'{what}: cameras [B{"" if new else "=%d" % self.cache.B},N,7] expected, got {tuple(cameras.shape)}')
        return cameras

    def _photo_codes(self, what, images, codes, B, views=None, shared: bool = False):
        """``images`` uint8 [B,P,H,W,3] (host or device; resized for the encoder as the evaluators do, encoded once; P = 0 encodes
        nothing) or ``codes`` [B,P,t,t] (exactly one of the two) -> int32 codes [B,P,t,t].  ``views``: the values P may take — (K,): one
        photo per camera, (1, N): one per camera or one per scene, None: any; ``shared``: the scene axis may also be 1 (one photo set for
        all scenes) -> [1,P,t,t].  Codes are integers (not bool, not floating point) of exactly that shape: nothing is reshaped or
        truncated on the caller's behalf."""
        if (images is None) == (codes is None):
            raise ValueError(f'{what}: exactly one of images / codes expected')
        cm, t = self.codebook, self.transformer.config.token_image_size
        scenes = (1, B) if shared else (B,)
        where = f'[{" or ".join(map(str, scenes))} scenes, {"any number of" if views is None else " or ".join(map(str, views))} views'
        if codes is None:
            images = torch.as_tensor(images).to(cm.device)
            if images.dim() != 5 or images.shape[0] not in scenes or (views is not None and images.shape[1] not in views):
                raise ValueError(f'{what}: images {where},H,W,3] expected, got {tuple(images.shape)}')
            S, P = images.shape[:2]
            codes = (cm.encode(_frames_for_encode(images, cm.config.image_size))[-1] if P
                     else torch.empty((S, 0, t, t), dtype=torch.int32, device=cm.device))
        else:
            codes = torch.as_tensor(codes).to(cm.device)
            if (codes.dim() != 4 or codes.shape[0] not in scenes or (views is not None and codes.shape[1] not in views)
                    or tuple(codes.shape[2:]) != (t, t) or codes.dtype.is_floating_point or codes.dtype == torch.bool):
                raise ValueError(f'{what}: codes int {where},{t},{t}] expected, got {codes.dtype} {tuple(codes.shape)}')
            S, P = codes.shape[:2]
        return codes.to(torch.int32).view(S, P, t, t)

    @staticmethod
    def _per_view(codes, N):
        """the photos of the views a ... b-1 of N: their own, or the scene's one photo for all of them"""
        one = codes.shape[1] == 1 and N > 1
        return lambda a, b: codes if one else codes[:, a:b]

    def _lengths(self, n_context, N):
        """the methods' ``n_context`` (an int, [B] or [B,N]; None: ``set_context``'s per-scene default) -> int32 [B,N] or None"""
        if n_context is None and self.n_context is None:
            return None                                                  # the rectangular path: nothing is asked of the cache
        return plan_context_lengths(n_context, self.cache.B, N, self.cache.C, scene_default=self.n_context)

    def _chunks(self, N, max_views_per_call, n_context):
        """[(a, b, keywords)] over the N views of every scene, in whole views (``plan_view_chunks``): the keywords are the chunk's slice
        of the context lengths as ``n_context=`` where lengths exist (``_lengths``), and nothing where they do not"""
        lens = self._lengths(n_context, N)
        return [(a, b, {} if lens is None else dict(n_context=lens[:, a:b])) for a, b in plan_view_chunks(N, self.cache.B, max_views_per_call)]

    def _walk(self, N, max_views_per_call, n_context, call, axis={}):
        """``call(a, b, **keywords)`` -> a dict, for every chunk of ``_chunks``; N = 0: the one call on the empty range, ``call(0, 0)``
        without a length keyword, for the empty tensors of the right shapes.  -> the parts concatenated key by key along axis 1 (the
        view axis; ``axis``: the keys whose view axis is another), a single part as it is"""
        parts = [call(a, b, **kw) for a, b, kw in self._chunks(N, max_views_per_call, n_context)]
        if not parts:
            parts = [call(0, 0)]
        return dict(parts[0]) if len(parts) == 1 else {k: torch.cat([p[k] for p in parts], axis.get(k, 1)) for k in parts[0]}

    def match(self, query_cameras, images=None, codes=None, max_views_per_call: int = None, n_context=None):
        """Which of M cameras does each of P photos belong to, and which photo does each camera expect?  ``query_cameras`` [B,M,7] in the
        caller's world frame (the context's) and ``images`` uint8 [B or 1,P,H,W,3] (host or device; resized for the encoder as the
        evaluators do, each photo encoded once) or ``codes`` int [B or 1,P,t,t] (already encoded; a scene axis of 1: one photo set for
        all scenes, e.g. ``bank.codes[None]``) -> ``MIGT.match_from_context``'s dict — log_likelihood, accuracy fp32 [B,P,M] (element
        [b,p,m] is ``score``'s for photo p at camera m, bit for bit; possibly a transposed view); predicted_codes, confidence, entropy
        [B,M,t,t] — plus
            best_camera  int64 [B,P]   the camera under which each photo is most likely
            best_photo   int64 [B,M]   the photo each camera's view makes most likely
        both the FIRST arg-max of log_likelihood (``ops.argmax_rows``: ties to the lowest index; -1 where there is nothing to choose
        from, M = 0 or P = 0).  The transformer runs M query views, not P x M.  M is walked in chunks of whole views
        (``plan_view_chunks``); an element does not depend on the chunking; P is not chunked.  ``n_context``: as ``render``'s, per camera."""
        self._context('match')
        query_cameras = self._world_cameras('match', query_cameras)
        B, M = self.cache.B, query_cameras.shape[1]
        codes = self._photo_codes('match', images, codes, B, shared=True)
        P = codes.shape[1]
        dev = query_cameras.device
        poses = query_poses(query_cameras, self.transform)
        res = self._walk(M, max_views_per_call, n_context,               # P is not chunked; the cameras are the last axis of [B,P,M]
                         lambda a, b, **lkw: self.transformer.match_from_context(self.cache, poses[:, a:b], codes, **lkw),
                         axis=dict(log_likelihood=2, accuracy=2))
        ll = res['log_likelihood']
        none = lambda n: torch.full((B, n), -1, dtype=torch.int64, device=dev)
        if M and P:
            res['best_camera'] = ops.argmax_rows(ll.contiguous().view(B * P, M), B * P, M).view(B, P)
            res['best_photo'] = ops.argmax_rows(ll.transpose(1, 2).contiguous().view(B * M, P), B * M, P).view(B, M)
        else:
            res['best_camera'], res['best_photo'] = none(P), none(M)
        return res

    def score_gradient(self, query_cameras, images=None, codes=None, max_views_per_call: int = None, n_context=None):
        """``score`` plus which way each camera should move: ``MIGT.score_grad_from_context``'s dict (``score``'s keys with the same
        bits, and grad_cameras fp32 [B,N,7]) plus ``poses`` fp32 [B,N,7], the MODEL-frame cameras (relative to context view 0 where the
        model was trained so, normalised) that the gradient refers to: grad_cameras[b,n] = d log_likelihood[b,n] / d poses[b,n].
        Arguments as ``score``'s; N is walked in chunks of whole views (``plan_view_chunks``), a view's result does not depend on the
        chunking."""
        self._context('score_gradient')
        self.cache.refuse_backward('ViewRenderer.score_gradient')
        query_cameras = self._world_cameras('score_gradient', query_cameras)
        N = query_cameras.shape[1]
        photo = self._per_view(self._photo_codes('score_gradient', images, codes, self.cache.B, (1, N)), N)
        poses = query_poses(query_cameras, self.transform)
        res = self._walk(N, max_views_per_call, n_context,
                         lambda a, b, **lkw: self.transformer.score_grad_from_context(self.cache, poses[:, a:b], photo(a, b), **lkw))
        res['poses'] = poses
        return res

    def refine(self, cameras0=None, images=None, codes=None, steps: int = 16, step_xyz: float = 0.05, step_rot: float = 0.05,
               max_views_per_call: int = None, n_context=None, return_trace: bool = False):
        """Refine camera estimates of N photos per scene by gradient ascent on their log-likelihood (``MIGT.refine_from_context``):
        ``cameras0`` [B,N,7] in the caller's world frame, or None to start from ``self.localize(...)`` of the same photos; ``images`` /
        ``codes`` as ``score``'s -> dict(generated_cameras fp32 [B,N,7] in the world frame, through ``from_relative_cameras`` as
        ``localize``; cameras [B,N,7] in the model's frame; log_likelihood, initial_log_likelihood fp32 [B,N]; accepted int32 [B,N]; with
        ``return_trace`` trace fp32 [steps+1,B,N]).  N is walked in chunks of whole views; views are refined independently of each other."""
        self._context('refine')
        self.cache.refuse_backward('ViewRenderer.refine')
        B = self.cache.B
        if cameras0 is not None:
            cameras0 = self._world_cameras('refine', cameras0)
        codes = self._photo_codes('refine', images, codes, B, None if cameras0 is None else (1, cameras0.shape[1]))
        if cameras0 is None:
            cameras0 = self.localize(codes=codes, max_views_per_call=max_views_per_call, n_context=n_context)['generated_cameras']
        N = cameras0.shape[1]
        photo = self._per_view(codes, N)
        poses = query_poses(cameras0, self.transform)
        kw = dict(steps=steps, step_xyz=step_xyz, step_rot=step_rot, return_trace=return_trace)
        res = self._walk(N, max_views_per_call, n_context,               # trace is [steps+1,B,N]
                         lambda a, b, **lkw: self.transformer.refine_from_context(self.cache, poses[:, a:b], photo(a, b), **kw, **lkw),
                         axis=dict(trace=2))
        cams = res['cameras']
        res['generated_cameras'] = geometry.from_relative_cameras(cams, self.transform) if self.transform is not None else cams
        return res

    def localize(self, images=None, codes=None, max_views_per_call: int = None, return_tokens: bool = False, n_context=None):
        """Estimate the cameras of N photos per scene against the context: ``images`` uint8 [B,N,H,W,3] (host or device; resized for
        the encoder as the evaluators do, each photo encoded once) or ``codes`` int [B,N,t,t] (already encoded, e.g.
        ``SceneBank.gather``) -> dict(generated_cameras fp32 [B,N,7]) in the caller's world frame (the context cameras'); with
        ``return_tokens`` also codes int32 [B,N,t,t], pose_prediction [B,N,L,7] (the per-token poses in the context's frame) and raw
        [B,N,L,7].  N is walked in chunks of whole views (``plan_view_chunks``).  ``n_context``: as ``render``'s."""
        self._context('localize')
        codes = self._photo_codes('localize', images, codes, self.cache.B)
        kw = dict(return_tokens=return_tokens, **({} if self.fused_tail is None else dict(fused_tail=bool(self.fused_tail))))

        def views(a, b, **lkw):                                          # (without return_tokens the model answers with the cameras alone)
            out = self.transformer.localize_from_context(self.cache, codes[:, a:b], **kw, **lkw)
            return out if return_tokens else dict(cameras=out)

        out = self._walk(codes.shape[1], max_views_per_call, n_context, views)
        cams = out['cameras']
        if self.transform is not None:                                   # evaluate_transformer.py:139-140
            cams = geometry.from_relative_cameras(cams, self.transform)
        res = dict(generated_cameras=cams)
        if return_tokens:
            res.update(codes=codes, pose_prediction=out['pose_prediction'], raw=out['raw'])
        return res

    def sweep(self, query_cameras, sizes=None, max_views_per_call: int = None, return_codes: bool = False):
        """The view at every camera from every context size: ``query_cameras`` [B,N,7] in the caller's world frame, ``sizes`` K integers
        in [0, C] (default 0 ... C; size 0 = no context photo at all) -> dict(generated_images uint8 [B,N,K,H,W,3], sizes int32 [K]);
        with ``return_codes`` also generated_codes int64 [B,N,K,t,t] and logits fp32 [B,N,K,t,t,n_embeddings].  ONE ``render`` over
        K N views laid out size-major (``sweep_layout``), from the one prefill: no context is encoded or prefilled per size.  After
        ``set_context(n_context=...)`` a size above a scene's number of valid views is that number (its padding is never read)."""
        self._context('sweep')
        B, C = self.cache.B, self.cache.C
        query_cameras = self._world_cameras('sweep', query_cameras)
        N = query_cameras.shape[1]
        sz = np.arange(C + 1) if sizes is None else _int_array('sweep: sizes', sizes)
        if sz.size and sz.max() > C:
            raise ValueError(f'sweep: sizes in [0, C={C}] expected, got {sizes}')
        sz = sz.astype(np.int32)
        K = sz.shape[0]
        cam, size, inverse = sweep_layout(N, K)
        lens = np.broadcast_to(sz[size].reshape(1, K * N), (B, K * N))
        if self.n_context is not None:
            lens = np.minimum(lens, self.n_context.reshape(B, 1))
        out = self.render(query_cameras[:, torch.from_numpy(cam).to(query_cameras.device)], max_views_per_call=max_views_per_call,
                          return_codes=return_codes, n_context=np.ascontiguousarray(lens, dtype=np.int32))
        back = torch.from_numpy(inverse.reshape(-1)).to(query_cameras.device)
        per_camera = lambda x: x[:, back].view(B, N, K, *x.shape[2:])
        res = dict(generated_images=per_camera(out['generated_images']), sizes=torch.from_numpy(sz))
        if return_codes:
            res.update(generated_codes=per_camera(out['generated_codes']), logits=per_camera(out['logits']))
        return res


def evaluate_context_sizes(transformer_model, codebook_model, images, cameras):
    """``evaluate_multictx.generate_batch_predictions`` from ONE cached context: ``images`` uint8 [B,S,H,W,3], ``cameras`` [B,S,7] -> the
    same keys and shapes — ground_truth_images, generated_images [B,S,H,W,3], ground_truth_cameras, generated_cameras [B,S,7],
    generated_codes [B,S,t,t], codes [B,S,t,t] — entry i being the last frame's view / pose from the first i frames as context.  All S
    frames are encoded once (as there); the S-1 context frames are prefilled once, the target camera is swept over the sizes 0 ... S-1
    and the target's code map is localized against the same sizes.  S = 1 leaves no context view: ValueError."""
    r = ViewRenderer(transformer_model, codebook_model)
    images = torch.as_tensor(images).to(codebook_model.device)
    cameras = r._world_cameras('evaluate_context_sizes', cameras, new=True)
    B, S = cameras.shape[:2]
    if S < 2:
        raise ValueError('evaluate_context_sizes: S >= 2 expected (S - 1 context views and the target)')
    t = transformer_model.config.token_image_size
    codes = r._photo_codes('evaluate_context_sizes', images, None, B, (S,))
    r.set_context(codes=codes[:, :-1], cameras=cameras[:, :-1])
    sizes = np.arange(S, dtype=np.int32)
    swp = r.sweep(cameras[:, -1:], sizes=sizes, return_codes=True)
    loc = r.localize(codes=codes[:, -1:].expand(B, S, t, t).contiguous(), n_context=sizes.reshape(1, S).repeat(B, 0))
    return dict(ground_truth_images=images[:, -1], generated_images=swp['generated_images'][:, 0],
                ground_truth_cameras=cameras[:, -1], generated_cameras=loc['generated_cameras'],
                generated_codes=swp['generated_codes'][:, 0], codes=codes)


def _with_context(transformer_model, codebook_model, images, cameras, kw, *names, **fixed):
    """A renderer with its context set, for the one-call functions: the keywords ``codes`` and ``names`` leave ``kw`` for ``set_context``
    (None where the caller gave none), ``fixed`` goes there as it is; what stays in ``kw`` is the method's."""
    ctx = {k: kw.pop(k, None) for k in ('codes', *names)}
    return ViewRenderer(transformer_model, codebook_model).set_context(images=images, cameras=cameras, **ctx, **fixed)


def render_views(transformer_model, codebook_model, images, cameras, query_cameras, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7] and ``query_cameras`` [B,N,7] -> ``ViewRenderer.render``'s
    dict.  Keywords: ``codes`` (context codes instead of images; pass images=None), ``max_views_per_call``, ``return_codes``."""
    r = _with_context(transformer_model, codebook_model, images, cameras, kw)
    return r.render(query_cameras, **kw)


def sweep_views(transformer_model, codebook_model, images, cameras, query_cameras, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7] and ``query_cameras`` [B,N,7] -> ``ViewRenderer.sweep``'s
    dict.  Keywords: ``codes`` (context codes instead of images; pass images=None), ``n_context`` (valid context views per scene),
    ``sizes``, ``max_views_per_call``, ``return_codes``."""
    r = _with_context(transformer_model, codebook_model, images, cameras, kw, 'n_context')
    return r.sweep(query_cameras, **kw)


def sample_views(transformer_model, codebook_model, images, cameras, query_cameras, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7] and ``query_cameras`` [B,N,7] -> ``ViewRenderer.sample``'s
    dict.  Keywords: ``codes`` (context codes instead of images; pass images=None), ``n_samples``, ``temperature``, ``top_k``, ``top_p``,
    ``seed``, ``max_views_per_call``, ``return_codes``."""
    r = _with_context(transformer_model, codebook_model, images, cameras, kw)
    return r.sample(query_cameras, **kw)


def mean_views(transformer_model, codebook_model, images, cameras, query_cameras, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7] and ``query_cameras`` [B,N,7] -> ``ViewRenderer.render_mean``'s
    dict.  Keywords: ``codes`` (context codes instead of images; pass images=None), ``temperature``, ``top_k``, ``top_p``,
    ``max_views_per_call``, ``return_latents``."""
    r = _with_context(transformer_model, codebook_model, images, cameras, kw)
    return r.render_mean(query_cameras, **kw)


def rollout_views(transformer_model, codebook_model, images, cameras, path_cameras, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7] and ``path_cameras`` [B,T,7] -> ``ViewRenderer.rollout``'s
    dict.  Keywords: ``codes`` (context codes instead of images; pass images=None), ``n_context`` (valid context views per scene),
    ``n_samples``, ``temperature``, ``top_k``, ``top_p``, ``seed``, ``return_codes``, ``fused_step``, ``pack`` (None, ``'kv'`` or
    ``'e4m3'``: roll out on a growing packed context, ``set_context(pack=...)``).  The cache is allocated with room for the whole path."""
    T = int(torch.as_tensor(path_cameras).shape[1])
    C = int(torch.as_tensor(cameras).shape[1])
    r = _with_context(transformer_model, codebook_model, images, cameras, kw, 'n_context', 'pack', capacity=C + T)
    return r.rollout(path_cameras, **kw)


def score_views(transformer_model, codebook_model, images, cameras, query_cameras, photos=None, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7], ``query_cameras`` [B,N,7] and ``photos`` uint8 [B,N,H,W,3] or
    [B,1,H,W,3] -> ``ViewRenderer.score``'s dict.  Keywords: ``codes`` (context codes instead of images; pass images=None), ``photo_codes``
    (the photos' codes instead of ``photos``), ``max_views_per_call``."""
    r = _with_context(transformer_model, codebook_model, images, cameras, kw)
    return r.score(query_cameras, images=photos, codes=kw.pop('photo_codes', None), **kw)


def match_views(transformer_model, codebook_model, images, cameras, query_cameras, photos=None, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7], ``query_cameras`` [B,M,7] and ``photos`` uint8
    [B or 1,P,H,W,3] -> ``ViewRenderer.match``'s dict (the [B,P,M] likelihoods from M query views, best_camera, best_photo).  Keywords:
    ``codes`` (context codes instead of images; pass images=None), ``photo_codes`` (the photos' codes instead of ``photos``),
    ``max_views_per_call``, ``n_context``."""
    r = _with_context(transformer_model, codebook_model, images, cameras, kw)
    return r.match(query_cameras, images=photos, codes=kw.pop('photo_codes', None), **kw)


def refine_views(transformer_model, codebook_model, images, cameras, photos=None, cameras0=None, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7], ``photos`` uint8 [B,N,H,W,3] and ``cameras0`` [B,N,7] (None:
    the localizer's estimate) -> ``ViewRenderer.refine``'s dict.  Keywords: ``codes`` (context codes instead of images; pass images=None),
    ``photo_codes`` (the photos' codes instead of ``photos``), ``steps``, ``step_xyz``, ``step_rot``, ``max_views_per_call``, ``return_trace``."""
    r = _with_context(transformer_model, codebook_model, images, cameras, kw)
    return r.refine(cameras0, images=photos, codes=kw.pop('photo_codes', None), **kw)


def localize_views(transformer_model, codebook_model, images, cameras, photos=None, **kw):
    """One call: context ``images`` uint8 [B,C,H,W,3] + ``cameras`` [B,C,7] and ``photos`` uint8 [B,N,H,W,3] -> ``ViewRenderer.localize``'s
    dict.  Keywords: ``codes`` (context codes instead of images; pass images=None), ``photo_codes`` (the photos' codes instead of
    ``photos``), ``max_views_per_call``, ``return_tokens``."""
    r = _with_context(transformer_model, codebook_model, images, cameras, kw)
    return r.localize(images=photos, codes=kw.pop('photo_codes', None), **kw)
