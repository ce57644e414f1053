"""The context cache of the novel-view renderer (MIGT.prefill_context), one class per storage form.

Every form owns its layout — which buffers it holds, their leading dimension and scene stride, what its ``capacity`` counts — in one
place and offers the same surface to ``MIGT``: ``plan_lengths`` / ``plan_pass`` (host-side, before any launch), ``append`` and
``attend`` (one launch each, per layer), ``attend_backward``, ``reserve`` / ``grown``, and ``replicate`` / ``fork`` / ``materialize`` /
``pack`` / ``unpack``, each of which BUILDS its result through the constructor of the result's form.  What a form cannot do it refuses
itself, naming the way out (``materialize()`` / ``unpack()``).  torch = memory only; every launch is an ``ops`` call."""
import copy
import weakref

import numpy as np
import torch

from . import ops


class ContextCache:
    """The PLAIN form — keys and values of C context views in every layer: ``kv[i]`` is layer i's fused c_attn output
    [B*capacity*L, 3*d_model] with thirds (V, Q, K), scenes capacity*L*3*d_model apart.  Valid for the model object, weights, arithmetic
    arm and device that made it.  ``capacity`` >= C views of room per scene (``prefill_context(capacity=...)``, grown by
    ``append_to_context``); ``C`` = the number of filled views, the maximum over scenes; ``lengths``: the filled views per scene, host
    int32 [B], or None for "all C" — tight, slack and ragged caches are this one form: lengths are data.  The other forms are its
    subclasses ``ForkedContextCache`` (``fork``), ``PackedKVCache`` and ``PackedE4M3Cache`` (``pack``), and the packed forms with room
    ``GrowingKVCache`` and ``GrowingE4M3Cache`` (``pack(room=...)``, ``prefill_context(pack=...)``)."""
    packed = None                     # None, 'kv' or 'e4m3'
    parent_kv = parent_capacity = split = share = room = _parent = _split_dev = None      # a fork's

    def __init__(self, model, kv, B, C, tshape, capacity=None, lengths=None):
        self.kv, self.B, self.C, self.tshape = kv, B, C, tuple(tshape)
        self.capacity = C if capacity is None else int(capacity)
        self.lengths = None if lengths is None else np.array(lengths, dtype=np.int32).reshape(B)
        self.device = model.device
        self.arm = (model.precision, model.dense_arith, model.attention)
        self.act16, self.qkv16 = model._act_dtypes()
        self.d, self.H, self.L = model.config.d_model, model.config.n_head, int(np.prod(self.tshape))
        self._owner = weakref.ref(model)
        self._weights = model._weights_version

    # ------------------------------------------------------------------ what every form says about itself
    def filled(self):
        """the filled views per scene, int32 [B] (host; a copy)"""
        return np.full(self.B, self.C, dtype=np.int32) if self.lengths is None else self.lengths.copy()

    def ragged(self):
        """True where the fixed-C attention entry would read unfilled rows: the cache has slack, or lengths of its own"""
        return self.capacity != self.C or self.lengths is not None

    def forked(self):
        """True for a cache made by ``fork``: two segments per scene, the parent's and its own"""
        return self.share is not None

    def alias(self):
        """A second cache of the same form on the SAME buffers with lengths of its own: what is appended through it lies beyond this
        cache's lengths (and moves to new buffers, leaving these, once the capacity is exceeded)."""
        c = copy.copy(self)
        c.kv = list(self.kv)
        c.lengths = None if self.lengths is None else self.lengths.copy()
        return c

    def nbytes(self):
        """the bytes of this cache's own tensors, from their shapes (a fork: its own buffers, not the parent's)"""
        return sum(x.numel() * x.element_size() for t in self.kv for x in (t if isinstance(t, tuple) else (t,)))

    def check(self, model):
        if self._owner() is not model or self._weights != model._weights_version:
            raise ValueError('ContextCache belongs to another model (or to weights that have been replaced since): prefill again')
        if self.arm != (model.precision, model.dense_arith, model.attention) or (self.act16, self.qkv16) != model._act_dtypes():
            raise ValueError(f'ContextCache was filled on the {self.arm} arm, the model now runs {(model.precision, model.dense_arith, model.attention)}')
        if self.device != model.device:
            raise ValueError(f'ContextCache lives on {self.device}, the model on {model.device}')

    def _model(self, what):
        m = self._owner()
        if m is None:
            raise ValueError(f'ContextCache.{what}: the model that filled this cache is gone')
        self.check(m)
        return m

    def refuse_packed(self, what):
        """``what`` grows, forks, copies or differentiates: a packed form refuses it"""

    def refuse_growth(self, what):
        """``what`` appends views: a packed form without room refuses it"""

    def refuse_backward(self, what):
        """``what`` needs ``attend_backward``: only the plain form has it"""

    # ------------------------------------------------------------------ one pass over query rows (MIGT._query_rows)
    def plan_lengths(self, n_context, N):
        """``n_context`` of the ``*_from_context`` methods -> the context length of every query view, host int32 [B,N], or None for the
        fixed-C attention entry (None in, on a form and a cache that can take it: no slack, no lengths of its own).  Anything but an
        int, [B] or [B,N] of integers in [0, the filled length of the scene]: ValueError."""
        from .render import plan_context_lengths
        if n_context is None:
            return plan_context_lengths(self.filled(), self.B, N, self.C) if self.ragged() else None
        plan = plan_context_lengths(n_context, self.B, N, self.C)
        if self.lengths is not None and plan.size and (plan > self.lengths.reshape(self.B, 1)).any():
            raise ValueError(f'n_context: at most the filled views of each scene ({self.lengths.tolist()}) expected, got {plan.max(1).tolist()}')
        return plan

    def plan_pass(self, n_context, append_at=None, save=None):
        """Before the first launch of a pass: refuse what this form cannot serve -> the positions ``append`` takes (``append_at``:
        None, or the logical views, int32 device tensor [B], at which the pass's views go into the cache)."""
        return append_at

    def append(self, i, qkv, N, at):
        """layer i: the V and K thirds of the N views per scene in ``qkv`` (fused c_attn rows [B*N*L, 3d]) to this cache's views
        ``at[b] + n`` (``plan_pass``'s positions) — one ``ops.kv_append``"""
        d, L, cap = self.d, self.L, self.capacity
        ops.kv_append(qkv, self.kv[i], self.B, N, L, d, 3 * d, 3 * d, cap * L * 3 * d, cap, at)

    def attend(self, i, qkv, att, N, ctx):
        """layer i: every query view of ``qkv`` attends to its ``ctx`` leading cached views (int32 device tensor [B*N]; None: all C, the
        fixed-C entry) and to itself -> ``att`` [B*N*L, d] — the one attention launch of this form"""
        d, L, cap, kv = self.d, self.L, self.capacity, self.kv[i]      # the attention's C is the room: lengths say what is filled
        ops.attn_prefix(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], kv[:, 2 * d:], kv[:, :d], att, self.B, self.H, cap, N, L,
                        3 * d, 3 * d, 3 * d, 3 * d, 3 * d, cap * L * 3 * d, d, bf16=self.arm[0] == 'bf16', ctx_len=ctx)

    def attend_backward(self, i, qkv, datt, dqkv, N, ctx):
        """layer i: ``ops.attn_prefix_bwd`` of ``attend`` over the query views; the cache is a constant (plain form only)"""
        d, L, cap, kv = self.d, self.L, self.capacity, self.kv[i]
        ops.attn_prefix_bwd(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], kv[:, 2 * d:], kv[:, :d], datt, dqkv, self.B, self.H, cap, N, L,
                            3 * d, 3 * d, 3 * d, 3 * d, 3 * d, cap * L * 3 * d, d, 3 * d, ctx_len=ctx)

    # ------------------------------------------------------------------ growing
    def reserve(self, needed):
        """room for ``needed`` (logical) views per scene: beyond the capacity, new buffers of max(2 capacity, needed) views
        (render.plan_capacity), inside the same object"""
        from .render import plan_capacity
        if needed > self.capacity:
            self.reallocate(plan_capacity(self.capacity, needed))

    def reallocate(self, capacity):
        """new buffers of ``capacity`` views per scene inside the same cache: every layer's cached views (the V and K thirds of all
        ``self.capacity`` views of every scene) copied bit for bit by one ``ops.kv_append`` at position 0"""
        d, L, B = self.d, self.L, self.B
        pos0 = torch.zeros(B, dtype=torch.int32, device=self.device)
        for i, src in enumerate(self.kv):
            dst = torch.empty((B * capacity * L, 3 * d), dtype=src.dtype, device=self.device)
            ops.kv_append(src, dst, B, self.capacity, L, d, 3 * d, 3 * d, capacity * L * 3 * d, capacity, pos0)
            self.kv[i] = dst
        self.capacity = capacity

    def grown(self, lengths, K):
        """K views were appended behind ``lengths`` (``filled()`` before the pass) in every scene"""
        if self.lengths is None:
            self.C += K
        else:
            self.lengths = (lengths + K).astype(np.int32)
            self.C = int(self.lengths.max())

    # ------------------------------------------------------------------ other forms of the same scenes
    def replicate(self, S):
        """a cache of B*S scenes, scene b's S copies at b*S ... b*S+S-1, in buffers of its own"""
        kv = [t.view(self.B, -1).repeat_interleave(S, 0).view(-1, t.shape[1]) for t in self.kv]
        return ContextCache(self._model('replicate'), kv, self.B * S, self.C, self.tshape, self.capacity,
                            None if self.lengths is None else np.repeat(self.lengths, S))

    def fork(self, S, room=None):
        """S children per scene that share this cache's views and own only what they add: a forked cache of B*S scenes, scene b's
        children at b*S ... b*S+S-1 (the order of ``render.plan_replication``), each starting at this cache's filled length of scene b.
        ``room``: own views of room per child (None: 0, allocated at the first append; grown by doubling, own buffers only).  Nothing of
        this cache is copied, written or run again, and nothing appended to it later — behind its lengths of now — reaches a child.
        ``generate`` / ``sample`` / ``score`` / ``localize_from_context``, ``append_to_context`` and ``rollout_from_context`` take the
        fork as any cache, with the bits of the materialised cache; ``score_grad_from_context`` and ``refine_from_context`` need
        ``materialize()``.  A fork of a fork is refused: ``materialize()`` it first."""
        from .render import plan_fork
        m = self._model('fork')
        m._check_render_shapes(self.L)                                       # an arm or shape without prefix-cache attention: refused whatever the cache
        if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= int(S) or self.B * int(S) > 65535:
            raise ValueError(f'fork: S, an integer >= 1 with B * S <= 65535, expected, got {S}')
        room = 0 if room is None else room
        if isinstance(room, bool) or not isinstance(room, (int, np.integer)) or int(room) < 0:
            raise ValueError(f'fork: room, an integer >= 0, expected, got {room}')
        S, room = int(S), int(room)
        split, _ = plan_fork(self.filled(), S)
        own = [torch.empty((self.B * S * room * self.L, 3 * self.d), dtype=kv.dtype, device=self.device) for kv in self.kv]
        return ForkedContextCache(m, own, self.B * S, self.tshape, split, list(self.kv), self.capacity, split, S, room, parent=self)

    def materialize(self):
        """A plain cache of this fork's B*S scenes in buffers of its own: the parent's views at position 0, the own views behind
        them, copied bit for bit by ``ops.kv_append`` (every result on it has the fork's bits).  On a plain cache: a copy."""
        return ContextCache(self._model('materialize'), [kv.clone() for kv in self.kv], self.B, self.C, self.tshape, self.capacity, self.lengths)

    def pack(self, dtype=None, room=None):
        """A packed, READ-ONLY cache of the same scenes in buffers of its own (this cache is left untouched), tight (capacity =
        the longest scene), lengths kept.  ``dtype=None``: the K and V thirds only, in the cache's dtype — 2/3 of the bytes, both arms,
        every result ``torch.equal`` to this cache's.  ``dtype='e4m3'`` (``precision='bf16'`` models only): OCP e4m3 bytes with one
        power-of-two scale per (scene, view, head) for K and one for V (``ops.kv_pack_e4m3``) — about 1/3 of the bf16 bytes; every
        result has the bits of the bf16 arm on ``unpack()``'s dequantised cache, and what is lost is the quantisation alone.
        ``generate`` / ``sample`` / ``score`` / ``localize_from_context`` take a packed cache as any cache; whatever grows a cache, forks
        it or differentiates through it refuses it: ``unpack()`` first.  A fork or a packed cache is refused: ``materialize()`` /
        ``unpack()`` first.
        ``room=R`` (an integer >= 0; opt-in): the GROWING packed form of the same ``dtype`` instead (``GrowingKVCache`` /
        ``GrowingE4M3Cache``) — ``capacity`` = C + R views per scene, the slack zero bytes (scales 1), and
        ``append_to_context`` / ``rollout_from_context`` take it; forks and gradients still need ``unpack()``."""
        m = self._model('pack')
        if dtype is not None and dtype != 'e4m3':
            raise ValueError(f"pack: dtype None (the K and V thirds as they are) or 'e4m3' expected, got {dtype!r}")
        if room is not None and (isinstance(room, bool) or not isinstance(room, (int, np.integer)) or int(room) < 0):
            raise ValueError(f'pack: room None (the tight, read-only pack) or an integer >= 0 expected, got {room!r}')
        if dtype == 'e4m3' and m.precision != 'bf16':
            raise ValueError(f"pack: dtype='e4m3' is for precision='bf16' models; the {m.precision!r} arm exists for exactness: "
                             'pack(dtype=None) keeps its bits')
        m._check_render_shapes(self.L)
        d, H, L, B, C, cap, dev = self.d, self.H, self.L, self.B, self.C, self.capacity, self.device
        lengths = self.filled() if self.ragged() else None                       # the length route whenever the source takes it
        if room is not None:
            return self._pack_with_room(m, dtype, C + int(room), lengths)
        if dtype is None:
            kvs = [tuple(kv.view(B, cap * L, 3 * d)[:, :C * L, a:a + d].contiguous().view(B * C * L, d) for a in (2 * d, 0)) for kv in self.kv]
            return PackedKVCache(m, kvs, B, C, self.tshape, lengths)
        filled = torch.from_numpy(self.filled()).to(dev)
        kvs = []
        for kv in self.kv:
            kq = torch.zeros((B * C, H, 64, 64), dtype=torch.uint8, device=dev)
            vq = torch.zeros((B * C, H, 64, 64), dtype=torch.uint8, device=dev)
            ks = torch.ones((B * C, H), dtype=torch.float32, device=dev)
            vs = torch.ones((B * C, H), dtype=torch.float32, device=dev)
            if B and C:
                ops.kv_pack_e4m3(kv, kq, vq, ks, vs, B, C, H, L, 3 * d, cap * L * 3 * d, filled)
            kvs.append((kq, vq, ks, vs))
        return PackedE4M3Cache(m, kvs, B, C, self.tshape, lengths)

    def _pack_with_room(self, m, dtype, capn, lengths):
        """``pack(dtype, room=capn - C)``: this cache's C leading views into fresh buffers of ``capn`` views per scene"""
        d, H, L, B, C, cap, dev = self.d, self.H, self.L, self.B, self.C, self.capacity, self.device
        if dtype is None:
            kvs = []
            for kv in self.kv:
                k, v = GrowingKVCache.buffers(B, capn, L, d, kv.dtype, dev)
                src = kv.view(B, cap * L, 3 * d)[:, :C * L]
                k.view(B, capn * L, d)[:, :C * L] = src[:, :, 2 * d:]
                v.view(B, capn * L, d)[:, :C * L] = src[:, :, :d]
                kvs.append((k, v))
            return GrowingKVCache(m, kvs, B, C, self.tshape, capn, lengths)
        filled = torch.from_numpy(self.filled()).to(dev)
        kvs = []
        for kv in self.kv:
            t = GrowingE4M3Cache.buffers(B, capn, H, dev)
            if B and C:
                ops.kv_pack_e4m3(kv, *t, B, C, H, L, 3 * d, cap * L * 3 * d, filled, q_scene_stride=capn * H * 4096, s_scene_stride=capn * H)
            kvs.append(t)
        return GrowingE4M3Cache(m, kvs, B, C, self.tshape, capn, lengths)

    def unpack(self):
        """A plain cache (thirds V, Q, K) of a packed one, in buffers of its own: the K and V thirds bit for bit (K/V-only form)
        or dequantised (e4m3 form: e4m3 * scale, exact in bf16), the Q third zeros — the way back to ``append_to_context``,
        ``rollout_from_context``, ``fork`` and the gradients.  On a cache that is not packed: refused."""
        self._model('unpack')
        raise ValueError('unpack: a packed cache (ContextCache.pack) expected')


class ForkedContextCache(ContextCache):
    """B = parents * ``share`` scenes that read the parent's views where they lie and own only what they add:
    ``parent_kv`` = the parent's per-layer tensors as they were at fork time (a list of its own: a parent that reallocates later keeps
    the old buffers alive for the child), ``parent_capacity`` their views of room per scene, ``split`` host int32 [B] = the parent's
    filled length per child scene at fork time, ``share`` = S (child scene b reads parent scene b // S), ``room`` = own views of room
    per child scene, and ``kv[i]`` the OWN buffers [B*room*L, 3*d_model].  ``filled()``, ``lengths``, ``C`` and ``capacity`` count
    LOGICAL views: logical view s of scene b is parent view s below ``split[b]``, own view ``s - split[b]`` otherwise
    (``render.map_fork_views``), and ``capacity`` = the longest split + ``room``.  Every child holds the same number of own views."""

    def __init__(self, model, kv, B, tshape, lengths, parent_kv, parent_capacity, split, share, room, parent=None):
        split = np.array(split, dtype=np.int32).reshape(B)
        super().__init__(model, kv, B, int(np.max(lengths)) if B else 0, tshape, (int(split.max()) if B else 0) + room, lengths)
        self.parent_kv, self.parent_capacity, self.split, self.share, self.room = parent_kv, parent_capacity, split, share, room
        self._parent = None if parent is None else weakref.ref(parent)       # adopt_from_fork asks for it
        self._split_dev = torch.from_numpy(split).to(self.device)

    def alias(self):
        c = super().alias()
        c.parent_kv = list(self.parent_kv)
        return c

    def refuse_backward(self, what):
        raise ValueError(f'{what}: the backward pass has no fork arm: pass cache.materialize() instead of the forked cache')

    def attend_backward(self, *args):
        self.refuse_backward('attend_backward')

    def plan_pass(self, n_context, append_at=None, save=None):
        if n_context is None:
            raise ValueError('_query_rows: a forked cache takes the length route')
        return None if append_at is None else append_at - self._split_dev    # lengths and positions are logical: own view = logical - split

    def append(self, i, qkv, N, at):
        d, L, room = self.d, self.L, self.room
        ops.kv_append(qkv, self.kv[i], self.B, N, L, d, 3 * d, 3 * d, room * L * 3 * d, room, at)

    def attend(self, i, qkv, att, N, ctx):
        d, L, Cp, room = self.d, self.L, self.parent_capacity, self.room
        pkv, own = self.parent_kv[i], self.kv[i]                             # [B/share*Cp*L, 3d], read where it lies; [B*room*L, 3d]
        own = (own[:, 2 * d:], own[:, :d]) if room else (None, None)
        ops.attn_prefix_fork(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], pkv[:, 2 * d:], pkv[:, :d], *own, att, self.B, self.H, Cp, room, N, L,
                             3 * d, 3 * d, 3 * d, 3 * d, 3 * d, Cp * L * 3 * d, 3 * d, 3 * d, room * L * 3 * d, d, ctx,
                             self._split_dev, self.share, bf16=self.arm[0] == 'bf16')

    def reserve(self, needed):
        """the own room doubles, not the logical capacity (the parent's part is not the fork's)"""
        from .render import plan_capacity
        if needed > self.capacity:
            base = int(self.split.max())
            self.reallocate(base + plan_capacity(self.room, needed - base))

    def reallocate(self, capacity):
        """a fork grows its OWN buffers only: the parent's stay where they lie"""
        d, L, B = self.d, self.L, self.B
        pos0 = torch.zeros(B, dtype=torch.int32, device=self.device)
        room = capacity - int(self.split.max())
        for i, src in enumerate(self.kv):
            dst = torch.empty((B * room * L, 3 * d), dtype=src.dtype, device=self.device)
            if self.room:
                ops.kv_append(src, dst, B, self.room, L, d, 3 * d, 3 * d, room * L * 3 * d, room, pos0)
            self.kv[i] = dst
        self.room, self.capacity = room, capacity

    def replicate(self, S):
        """the own buffers are copied, the parent's still shared: (b S + s) // (share S) = b // share"""
        kv = [t.view(self.B, -1).repeat_interleave(S, 0).view(-1, t.shape[1]) for t in self.kv]
        return ForkedContextCache(self._model('replicate'), kv, self.B * S, self.tshape, np.repeat(self.lengths, S), list(self.parent_kv),
                                  self.parent_capacity, np.repeat(self.split, S), self.share * S, self.room)

    def fork(self, S, room=None):
        self._model('fork')
        raise ValueError('fork: a fork of a fork is not supported: fork cache.materialize() instead')

    def pack(self, dtype=None, room=None):
        self._model('pack')
        raise ValueError('pack: a forked cache reads two segments: pack cache.materialize() instead')

    def materialize(self):
        m = self._model('materialize')
        d, L, B, dev = self.d, self.L, self.B, self.device
        S, Bp, Cp, room = self.share, self.B // self.share, self.parent_capacity, self.room
        cap = self.capacity                                                  # split.max() + room: every logical view has its place
        pos0 = torch.zeros(Bp, dtype=torch.int32, device=dev)
        kvs = []
        for pkv, own in zip(self.parent_kv, self.kv):
            dst = torch.empty((B * cap * L, 3 * d), dtype=own.dtype, device=dev)
            for s in range(S):                                               # the parent's views to child s of every scene (views beyond cap are skipped)
                ops.kv_append(pkv, dst[s * cap * L:], Bp, Cp, L, d, 3 * d, 3 * d, S * cap * L * 3 * d, cap, pos0)
            if room:                                                         # the own views behind each scene's split, over whatever the parent held there
                ops.kv_append(own, dst, B, room, L, d, 3 * d, 3 * d, cap * L * 3 * d, cap, self._split_dev)
            kvs.append(dst)
        return ContextCache(m, kvs, B, self.C, self.tshape, cap, self.lengths)


class PackedKVCache(ContextCache):
    """READ-ONLY, no Q third, tight (``capacity`` = ``C``, the longest scene): ``kv[i]`` = (K, V), two contiguous
    [B*C*L, d_model] tensors in the cache's dtype, served by the plain prefix attention with the bits of the source cache."""
    packed = 'kv'

    def __init__(self, model, kv, B, C, tshape, lengths=None):
        super().__init__(model, kv, B, C, tshape, None, lengths)

    def refuse_packed(self, what):
        raise ValueError(f'{what}: a packed cache is read-only (it holds no Q third and has no room): pass cache.unpack() instead')

    refuse_backward = refuse_growth = refuse_packed

    def _refuse(self, what):
        self._model(what)
        self.refuse_packed(what)

    def plan_pass(self, n_context, append_at=None, save=None):
        if append_at is not None or save is not None:
            raise ValueError('_query_rows: a packed cache is read-only and has no backward pass: unpack() first')

    def attend(self, i, qkv, att, N, ctx):
        d, L, C = self.d, self.L, self.capacity
        k, v = self.kv[i]                                                    # each [B*C*L, d] — the source cache's values, its bits
        ops.attn_prefix(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], k, v, att, self.B, self.H, C, N, L,
                        3 * d, 3 * d, 3 * d, d, d, C * L * d, d, bf16=self.arm[0] == 'bf16', ctx_len=ctx)

    def _read_only(self, *args):
        self.refuse_packed('ContextCache')

    append = attend_backward = reserve = reallocate = _read_only

    def replicate(self, S):
        self._refuse('replicate')

    def fork(self, S, room=None):
        self._refuse('fork')

    def materialize(self):
        self._refuse('materialize')

    def pack(self, dtype=None, room=None):
        self._model('pack')
        raise ValueError(f'pack: this cache is packed already ({self.packed!r}): pack cache.unpack() instead')

    def _thirds(self, dt):
        """(K, V) of every layer, each [B*capacity*L, d] in the plain form's dtype ``dt``"""
        return self.kv

    def unpack(self):
        m = self._model('unpack')
        dt = torch.bfloat16 if self.qkv16 else torch.float32
        kvs = []
        for k, v in self._thirds(dt):
            kv = torch.zeros((self.B * self.capacity * self.L, 3 * self.d), dtype=dt, device=self.device)
            kv[:, 2 * self.d:], kv[:, :self.d] = k, v
            kvs.append(kv)
        return ContextCache(m, kvs, self.B, self.C, self.tshape, self.capacity, self.lengths)


class PackedE4M3Cache(PackedKVCache):
    """The e4m3 pack (bf16 arm): ``kv[i]`` = (kq uint8 [B*C, H, 64 keys, 64 features], vq uint8 [B*C, H, 64 features, 64 keys], kscale,
    vscale fp32 [B*C, H]) — OCP e4m3 bytes with one power-of-two scale per (scene, view, head), served by ``ops.attn_prefix_q8`` with
    the bits of the bf16 arm on the dequantised cache (``unpack()``)."""
    packed = 'e4m3'

    def plan_lengths(self, n_context, N):
        """(the e4m3 attention is a length kernel: its default lengths are all C)"""
        return super().plan_lengths(self.filled() if n_context is None else n_context, N)

    def plan_pass(self, n_context, append_at=None, save=None):
        super().plan_pass(n_context, append_at, save)
        if n_context is None or self.arm[0] != 'bf16':
            raise ValueError('_query_rows: an e4m3 cache takes the length route of the bf16 arm')

    def attend(self, i, qkv, att, N, ctx):
        d = self.d
        ops.attn_prefix_q8(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], *self.kv[i], att, self.B, self.H, self.capacity, N, self.L, 3 * d, 3 * d, 3 * d, d, ctx)

    def _thirds(self, dt):
        """byte -> value through the 256 e4m3 numbers (exact), times the tile's scale"""
        n = self.B * self.capacity
        lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(self.device)
        for kq, vq, ks, vs in self.kv:
            k = lut[kq.long()] * ks.view(n, self.H, 1, 1)                    # [B*C, H, key, feature]
            v = lut[vq.long()] * vs.view(n, self.H, 1, 1)                    # [B*C, H, feature, key]
            yield k.permute(0, 2, 1, 3).reshape(n * self.L, self.d).to(dt), v.permute(0, 3, 1, 2).reshape(n * self.L, self.d).to(dt)


class _Growing:
    """What the two packed forms WITH ROOM share: ``capacity`` >= ``C`` views of room per scene in every tensor,
    lengths as data (the plain form's ``filled`` / ``ragged`` / ``grown``), ``append`` as ONE launch of the form's own append kernel at
    each scene's own length, the parent form's ``attend`` with ``capacity`` as the attention's C, and ``reserve`` / ``reallocate`` by
    ``render.plan_capacity`` with one strided device copy per tensor.  Forks, ``materialize``, ``pack`` and the backward pass refuse as
    on every packed cache and name ``unpack()``, which gives a plain cache of the same capacity and lengths."""

    def refuse_packed(self, what):
        raise ValueError(f'{what}: a packed cache holds no Q third (it grows, but it cannot be forked, copied to a plain one or '
                         'differentiated through): pass cache.unpack() instead')

    refuse_backward = refuse_packed

    def refuse_growth(self, what):
        """(``append_to_context`` and ``rollout_from_context`` are what this form is for)"""

    def plan_pass(self, n_context, append_at=None, save=None):
        if save is not None:
            self.refuse_backward('_query_rows')
        return append_at

    reserve = ContextCache.reserve

    def reallocate(self, capacity):
        """new buffers of ``capacity`` views per scene inside the same cache: every tensor's ``self.capacity`` views of every scene
        moved by one strided copy, bit for bit (bytes and scales included); the new slack as ``buffers`` leaves it"""
        B, old = self.B, self.capacity
        for i, ts in enumerate(self.kv):
            new = self._buffers(capacity, ts[0].dtype)
            for dst, src in zip(new, ts):
                dst.view(B, capacity, -1)[:, :old] = src.view(B, old, -1)
            self.kv[i] = new
        self.capacity = capacity

    def replicate(self, S):
        kv = [tuple(t.view(self.B, -1).repeat_interleave(S, 0).view(-1, *t.shape[1:]) for t in ts) for ts in self.kv]
        return type(self)(self._model('replicate'), kv, self.B * S, self.C, self.tshape, self.capacity,
                          None if self.lengths is None else np.repeat(self.lengths, S))


class GrowingKVCache(_Growing, PackedKVCache):
    """The K/V-only pack WITH ROOM: ``kv[i]`` = (K, V), two contiguous [B*capacity*L, d_model] tensors in the cache's
    dtype, scenes capacity*L*d_model apart — the plain cache's own K and V values, appended by ``ops.kv_append_split`` and walked by the
    plain prefix attention with ld d: every answer ``torch.equal`` to the answer of a plain cache grown the same way."""

    def __init__(self, model, kv, B, C, tshape, capacity, lengths=None):
        ContextCache.__init__(self, model, kv, B, C, tshape, capacity, lengths)

    @staticmethod
    def buffers(B, capacity, L, d, dtype, device):
        """one layer's (K, V) with room for ``capacity`` views per scene, zeros"""
        return tuple(torch.zeros((B * capacity * L, d), dtype=dtype, device=device) for _ in range(2))

    def _buffers(self, capacity, dtype):
        return self.buffers(self.B, capacity, self.L, self.d, dtype, self.device)

    def append(self, i, qkv, N, at):
        d, L, cap = self.d, self.L, self.capacity
        k, v = self.kv[i]
        ops.kv_append_split(qkv, k, v, self.B, N, L, d, 3 * d, d, d, cap * L * d, cap * L * d, cap, at)


class GrowingE4M3Cache(_Growing, PackedE4M3Cache):
    """The e4m3 pack WITH ROOM (bf16 arm): ``kv[i]`` = (kq, vq uint8 [B*capacity, H, 64, 64], kscale, vscale fp32
    [B*capacity, H]).  A new view brings its own tiles and scales (``ops.kv_append_e4m3``, the pack kernel's tile routine) and touches
    nothing that is stored; ``ops.attn_prefix_q8`` reads the buffers with ``capacity`` as its C."""

    def __init__(self, model, kv, B, C, tshape, capacity, lengths=None):
        ContextCache.__init__(self, model, kv, B, C, tshape, capacity, lengths)

    @staticmethod
    def buffers(B, capacity, H, device):
        """one layer's (kq, vq, kscale, vscale) with room for ``capacity`` views per scene: zero bytes, scales 1"""
        return (torch.zeros((B * capacity, H, 64, 64), dtype=torch.uint8, device=device),
                torch.zeros((B * capacity, H, 64, 64), dtype=torch.uint8, device=device),
                torch.ones((B * capacity, H), dtype=torch.float32, device=device),
                torch.ones((B * capacity, H), dtype=torch.float32, device=device))

    def _buffers(self, capacity, dtype):
        return self.buffers(self.B, capacity, self.H, self.device)

    def plan_pass(self, n_context, append_at=None, save=None):
        at = _Growing.plan_pass(self, n_context, append_at, save)
        if n_context is None or self.arm[0] != 'bf16':
            raise ValueError('_query_rows: an e4m3 cache takes the length route of the bf16 arm')
        return at

    def append(self, i, qkv, N, at):
        ops.kv_append_e4m3(qkv, *self.kv[i], self.B, N, self.H, self.L, 3 * self.d, self.capacity, at)


class PrefillSink:
    """What ``MIGT._blocks`` takes as ``kv_sink`` when ``prefill_context(pack=...)`` fills a growing packed cache directly: ``_blocks``
    hands over each layer's fused c_attn buffer BEFORE it launches the GEMM that fills it, so the buffer of layer i is appended to the
    cache (at position 0, one launch) when layer i + 1's arrives — stream order puts that behind the GEMM — or at ``close()``, and is
    dropped then: the plain cache of all layers never exists."""

    def __init__(self, cache, C):
        self.cache, self.C, self.layer, self.pending = cache, C, 0, None
        self.pos0 = torch.zeros(cache.B, dtype=torch.int32, device=cache.device)

    def append(self, qkv):
        self.close()
        self.pending = qkv

    def close(self):
        if self.pending is not None:
            self.cache.append(self.layer, self.pending, self.C, self.pos0)
            self.layer, self.pending = self.layer + 1, None
