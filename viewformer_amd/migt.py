"""MIGT image-token transformer on MI355X — host-side mirror of the reference model object.

Protocol (reference viewformer/models/migt.py:241-455):
``model(dict(input_ids=[B,S,t,t] int, poses=[B,S or S-1,7] f32), training=False)
  -> dict(logits=[B,S,t,t,n_embeddings] f32, pose_prediction=[B,S,L,7] (if use_localization),
          hidden_states=[...])``, attributes ``mask_token``, ``use_localization``, ``config``,
``reduce_cameras(x, axis)``.  Inference graph only in this file (single stream:
evaluate_transformer.py:119-123,134-136); the multi-stream training/multictx graph is a
"next" row.

All arithmetic runs in libvf_hip.so: embedding-sum, LayerNorm, fused c_attn GEMM whose V|Q|K
thirds are read in place by the block-causal attention kernel, c_proj/MLP GEMMs with fused
bias / exact-erf GELU / residual epilogues, tied LM head.  torch = memory + stream only
(plus O(B*S) pose bookkeeping on [B,S,7] tensors).
"""
from collections import OrderedDict

import math
import os

import numpy as np
import torch

from . import ops
from . import geometry
from .config import MIGTConfig
from .context_cache import ContextCache, GrowingKVCache, GrowingE4M3Cache, PrefillSink      # noqa: F401  (tests and tools import ContextCache from here)


ARMS = ('bf16', 'x3h', 'x6', 'f32')      # a dense launch's arithmetic (ops.ARM_KW), fastest first


class _Dense:
    """one dense layer [k] -> [n]: raw weight, bias, and its packings keyed by arm — ``packed`` for x @ W, ``packed_T`` for dy @ W^T
    (``w_raw_T``: the unpacked transpose, _pose_embed_bwd).  The caches live and die with the record: new weights, new records."""
    __slots__ = ('k', 'n', 'bias', 'w_raw', 'packed', 'packed_T', 'w_raw_T')

    def __init__(self, k, n, w_raw=None, bias=None):
        self.k, self.n, self.w_raw, self.bias = k, n, w_raw, bias
        self.packed, self.packed_T, self.w_raw_T = {}, {}, None


def dense_arm(d):
    """the arm of a forward launch of record ``d``: the fastest it holds a packing for"""
    return next(a for a in ARMS if a in d.packed)


class MIGT:
    def __init__(self, config: MIGTConfig = None, device=None, skip_masked: bool = True, precision: str = 'f32',
                 dense_arith: str = 'x3h', bf16_activations: bool = True, attention: str = None):
        """``dense_arith`` picks how the fp32 dense layers are evaluated (precision='f32' only): 'f32' = native f32 MFMA,
        'x6' = the fp32-EQUIVALENT six-term split-bf16 GEMM (csrc/gemm_x6.hip: same error against fp64, ~1.8x faster),
        'x3h' = the three-term split-fp16 GEMM (csrc/gemm_x3h.hip: same error for activations in fp16's range — LayerNorm / GELU /
        attention outputs are —, half the matrix instructions; attention stays x6).
        ``precision='bf16'``: the dense layers (c_attn, c_proj, MLP, LM head, pose MLPs) run on the bf16-MFMA arm with
        fp32 activations / accumulation, and the attention contractions (q.k^T, p.v) on bf16 MFMA with an fp32 softmax;
        LayerNorm, the residual stream and the arg-max stay fp32.
        Logits are then tolerance-bounded (tests state the bound), as the north star allows for the transformer.
        ``_upload`` decides which arms a layer (``_dense[name]``) and the tied LM head (``_head``) keep a packing for; ``dense_arm``
        picks a launch's arm from them, and nothing else does."""
        assert precision in ('f32', 'bf16') and dense_arith in ('f32', 'x6', 'x3h') and attention in (None, 'bf16', 'fp8')
        if attention is not None and precision != 'bf16':
            raise ValueError("attention='bf16' / 'fp8' belong to the tolerance arm: use precision='bf16'")
        # ``attention='fp8'`` (BASELINE configs[4]): q.k^T and p.v on v_mfma_f32_32x32x16_fp8_fp8 with OCP e4m3 operands, fp32 softmax
        # (csrc/attention_lp.hip); the dense layers stay on the bf16 arm.  Tolerances: tests/test_hip_fp8.py.
        self.attention = attention or ('bf16' if precision == 'bf16' else 'f32')
        self.precision = precision
        self.dense_arith = dense_arith
        # bf16 arm only: LayerNorm / GELU / attention outputs — values that only bf16 GEMMs consume — are written as bf16 by their
        # producers (exactly the rounding the GEMM would apply on load: bit-identical logits, half the traffic of the widest tensors)
        self.bf16_activations = bf16_activations
        self.config = config or MIGTConfig()
        c = self.config
        self.n_image_tokens = c.token_image_size ** 2
        self.mask_token = c.n_embeddings                      # migt.py:256
        self.localization_token = c.n_embeddings + 1          # migt.py:257
        self.use_localization = c.use_localization            # migt.py:269
        self.device = torch.device(device) if device is not None else None
        self.skip_masked = skip_masked
        self._sd_host = None
        self._dense = {}
        self._ln = {}
        self._weights_version = 0                             # counts uploads: a ContextCache is tied to the weights that filled it

    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise ops._lib.VfError('viewformer_amd.MIGT runs on the GPU only (no CPU fallback)')
        self.device = device
        if self._sd_host is not None:
            self._upload()
        return self

    def expected_keys(self):
        c = self.config
        keys = ['wte.weight', 'wpe.embeddings']
        dense = ['pose_embedding.c_fc', 'pose_embedding.c_proj',
                 'pose_criterion.pose_classifier.c_fc', 'pose_criterion.pose_classifier.c_proj']
        lns = ['ln_f']
        for i in range(c.n_layer):
            dense += [f'h.{i}.attn.c_attn', f'h.{i}.attn.c_proj', f'h.{i}.mlp.c_fc', f'h.{i}.mlp.c_proj']
            lns += [f'h.{i}.ln_1', f'h.{i}.ln_2']
        for d in dense:
            keys += [d + '.weight', d + '.bias']
        for l in lns:
            keys += [l + '.gamma', l + '.beta']
        if c.use_dynamic_pose_loss:
            # DynamicLossWeightingCriterion (migt.py:105-112) is built whenever the flag is set (:279-280), localization head or not,
            # so a checkpoint of such a model always carries the pair; only the training step reads it
            keys.append('pose_loss_weighting_criterion.pos_ori_weights')
        return keys

    _DYN_KEY = 'pose_loss_weighting_criterion.pos_ori_weights'

    def load_state_dict(self, state_dict, strict: bool = True):
        # the one training-only variable (DynamicLossWeightingCriterion, migt.py:105-112, initial value [0, -3]) is tolerated either way:
        # state dicts written before the key was tracked lack it, and a Keras checkpoint of a model trained with the flag carries it
        # even when the loading config has the flag off (inference never reads it)
        if strict and (self._DYN_KEY in state_dict) != bool(self.config.use_dynamic_pose_loss):
            state_dict = OrderedDict(state_dict)
            if self.config.use_dynamic_pose_loss:
                state_dict[self._DYN_KEY] = np.array([0.0, -3.0], dtype=np.float32)
            else:
                del state_dict[self._DYN_KEY]
        if strict:
            want, have = set(self.expected_keys()), set(state_dict.keys())
            if want - have:
                raise RuntimeError(f'Missing keys: {want - have}')
            if have - want:
                raise RuntimeError(f'Unexpected keys: {have - want}')
        host = OrderedDict()
        for k, v in state_dict.items():
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            host[k] = np.ascontiguousarray(v).reshape(-1) if k.endswith('.bias') else np.ascontiguousarray(v)
        self._sd_host = host
        if self.device is not None:
            self._upload()
        return self

    def state_dict(self):
        return OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in self._sd_host.items())      # copies: host arrays may be read-only views

    def _upload(self):
        dev, h, c = self.device, self._sd_host, self.config

        def dev_t(name):
            return torch.from_numpy(h[name]).to(dev, torch.float32).contiguous()

        fast = 'bf16' if self.precision == 'bf16' else self.dense_arith if self.dense_arith != 'f32' else None
        arms = lambda native, wide: ('f32',) * native + (fast,) * bool(fast and wide)      # noqa: E731  (native first: the order they are packed in)

        def dense(name, pack=True):
            w = dev_t(name + '.weight')
            d = self._dense[name] = _Dense(*w.shape, w, dev_t(name + '.bias'))
            d.packed = {a: ops.pack_dense(a, w) for a in arms(d.k % 32 == 0, d.k % 64 == 0 and d.n >= 64) if pack}

        def ln(name):
            self._ln[name] = (dev_t(name + '.gamma'), dev_t(name + '.beta'))

        self._wte = dev_t('wte.weight')
        self._wpe = dev_t('wpe.embeddings')
        # the tied LM head as a layer d_model -> n_embeddings whose weight lies transposed: logits sliced to n_embeddings (migt.py:417)
        self._head = _Dense(c.d_model, c.n_embeddings, self._wte[:c.n_embeddings])
        self._head.packed = {a: ops.pack_dense(a, self._wte, True, c.n_embeddings) for a in arms(True, c.d_model % 64 == 0)}
        dense('pose_embedding.c_fc', pack=False)
        dense('pose_embedding.c_proj')
        dense('pose_criterion.pose_classifier.c_fc')
        dense('pose_criterion.pose_classifier.c_proj')
        for i in range(c.n_layer):
            ln(f'h.{i}.ln_1'); ln(f'h.{i}.ln_2')
            for p in ('attn.c_attn', 'attn.c_proj', 'mlp.c_fc', 'mlp.c_proj'):
                dense(f'h.{i}.{p}')
        ln('ln_f')
        self._weights_version += 1
        torch.cuda.synchronize(dev)

    # ------------------------------------------------------------------ helpers
    def _gemm(self, x, name, M, epilogue=ops.EPI_NONE, res=None, out_bf16=False):
        d = self._dense[name]
        out = torch.empty((M, d.n), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
        self._dense_launch(x, d, M, out, res=res, epilogue=epilogue)
        return out

    @staticmethod
    def _dense_launch(x, d, M, out, res=None, epilogue=ops.EPI_NONE):
        """one dense layer on the arm ``dense_arm`` picks: bf16 (tolerance arm) > x3h, x6 (fp32-equivalent) > native f32 MFMA"""
        arm = dense_arm(d)
        ops.igemm(x, d.packed[arm], M, d.k, d.n, out, bias=d.bias, res=res, epilogue=epilogue, **ops.ARM_KW[arm], a16=x.dtype == torch.bfloat16,
                  o16=out.dtype == torch.bfloat16)

    def _lm(self, h, M, out):
        """tied LM head: logits = h @ wte[:n_embeddings]^T  (SharedEmbeddings._linear, migt.py:51-56,417)"""
        d, arm = self._head, dense_arm(self._head)
        ops.igemm(h, d.packed[arm], M, d.k, d.n, out, **ops.ARM_KW[arm])
        return out

    def _lm_argmax(self, h, M):
        """arg-max of the tied LM head WITHOUT materialising the logits (fused epilogue, csrc/lmhead_argmax.hip; bf16 arm): the codes
        ``tf.argmax(logits, -1)`` would give (evaluate_transformer.py:123), or None where the fused form does not apply (fp32 arm,
        odd shapes) — callers then compute the logits and call ops.argmax_rows."""
        c = self.config
        if 'bf16' not in self._head.packed or not ops.lmhead_argmax_supported(c.d_model, c.n_embeddings):
            return None
        return ops.lmhead_argmax_bf16(h, self._head.packed['bf16'], M, c.d_model, c.n_embeddings)

    def _lm_score(self, hf, M, target=None, fused: bool = False, want=ops.SCORE_OUTPUTS):
        """soft-max statistics of the tied LM head per row (ops.SCORE_OUTPUTS: first arg-max, its logit, log-sum-exp, the logit of
        ``target`` int32 [M], entropy) -> dict of [M] tensors.  Default: ``_lm`` then the row kernel on its logits (ops.logits_score).
        ``fused=True`` on the bf16 arm at a supported shape: the statistics in the head's epilogue, the logits never written
        (csrc/lmhead_score.hip) — measured slower than the default on the MI355X at 64 and at 8192 rows (every workgroup
        streams the whole packed wte), hence not the default; on every other arm and shape ``fused=True`` takes the default route.  There
        is no third route."""
        c = self.config
        if fused and 'bf16' in self._head.packed and ops.lmhead_score_supported(c.d_model, c.n_embeddings):
            return ops.lmhead_score_bf16(hf, self._head.packed['bf16'], M, c.d_model, c.n_embeddings, target=target, want=want)
        lg = torch.empty((M, c.n_embeddings), dtype=torch.float32, device=hf.device)
        self._lm(hf, M, lg)                                                  # migt.py:417
        return ops.logits_score(lg, M, c.n_embeddings, target=target, want=want)

    def _pose_embed(self, poses):
        """pose_embedding(get_model_input(poses)) — migt.py:139-145,291,354 (fp32; multiplier 1 at inference)"""
        B, Sp, _ = poses.shape
        c = self.config
        pin = geometry.pose_model_input(poses, c.pose_multiplier).reshape(B * Sp, 7).contiguous()
        fc = self._dense['pose_embedding.c_fc']
        h1 = ops.dense_small_k(pin, fc.w_raw, fc.bias, B * Sp, 7, fc.n, gelu=True)
        return self._gemm(h1, 'pose_embedding.c_proj', B * Sp).view(B, Sp, c.d_model)

    def reduce_cameras(self, cameras, axis=-2):
        """MIGT.reduce_cameras, migt.py:532-533"""
        return geometry.reduce_cameras(cameras, axis)

    prune_last_block = True           # callers that read only the last views' hidden states (generate_and_localize: the MASK and LOC views) get the LAST
                                      # block's projection, LayerNorm, MLP and ln_f on those views' rows only: every earlier block needs all rows (they are the
                                      # keys and values of the next block), the last block's other rows feed nothing.  Row for row the same launches on fewer
                                      # rows (GEMM rows, LayerNorm rows are independent of each other): the rows that are returned keep their bits

    def _act_dtypes(self):
        """(act16, qkv16): whether LayerNorm / GELU / attention outputs, and the fused c_attn output, are bf16 tensors in this arm"""
        c = self.config
        d = c.d_model
        l0 = self._dense['h.0.mlp.c_proj'] if c.n_layer else None
        act16 = (self.precision == 'bf16' and self.bf16_activations and d % 128 == 0 and l0 is not None and l0.k % 128 == 0
                 and all('bf16' in self._dense[f'h.{i}.{n}'].packed for i in range(c.n_layer)
                         for n in ('attn.c_attn', 'attn.c_proj', 'mlp.c_fc', 'mlp.c_proj')))
        # the fused c_attn output is bf16 too (bit-identical downstream: the attention kernel rounds fp32 q/k/v to bf16 on load): half
        # the bytes written by the GEMM and read by the attention, whose LDS-DMA kernel (attention_dma.hip) takes bf16 tiles straight
        # into LDS.  VF_QKV16=0 keeps fp32 q/k/v (A/B runs).
        # (the fp8 arm's kernel stages its tiles through registers and takes fp32 q/k/v at full speed: no bf16 there)
        qkv16 = act16 and self.attention != 'fp8' and os.environ.get('VF_QKV16', '1') != '0'
        return act16, qkv16

    def _blocks(self, ids, add_emb, B, V, L, mask_spec=-1, tail_views=0, kv_sink=None):
        """embedding sum -> n_layer x Block -> ln_f over V views of L tokens.  ids [B,V,...] int,
        add_emb [B,V,d] (pose embedding or LOC-token row per view).  Returns [B*V*L, d]; with ``tail_views`` = k > 0 (and prune_last_block)
        the hidden states of the last k views only, [B*k*L, d].  ``kv_sink``: a list that receives every layer's fused c_attn output
        [B*V*L, 3d] (thirds V, Q, K), each in a buffer of its own."""
        c, dev = self.config, self.device
        d, H = c.d_model, c.n_head
        T, M = V * L, B * V * L
        add = add_emb.contiguous().view(B * V, d)
        ids32 = ids.reshape(M).to(torch.int32).contiguous()
        h = ops.embed_sum(ids32, self._wte, self._wpe, add, B * V, L, d, c.n_embeddings + 2)   # migt.py:392
        act16, qkv16 = self._act_dtypes()
        att = torch.empty((M, d), dtype=torch.bfloat16 if act16 else torch.float32, device=dev)
        qkv = torch.empty((M, 3 * d), dtype=torch.bfloat16 if qkv16 else torch.float32, device=dev)
        for i in range(c.n_layer):                                           # Block.call, migt.py:230-238
            p = f'h.{i}'
            a = ops.layernorm(h, *self._ln[p + '.ln_1'], M, d, out_bf16=act16)
            ca = self._dense[p + '.attn.c_attn']
            if kv_sink is not None:                                          # prefill_context: every layer keeps its c_attn output (the K / V cache)
                if i:
                    qkv = torch.empty_like(qkv)
                kv_sink.append(qkv)
            self._dense_launch(a, ca, M, qkv)
            # thirds are (V, Q, K): migt.py:207-213
            ops.attn_blockcausal(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], att, B, H, T, L,
                                 3 * d, 3 * d, 3 * d, d, 1.0, self.skip_masked, mask_spec, bf16=self.precision == 'bf16',
                                 x6=self.precision == 'f32' and self.dense_arith in ('x6', 'x3h'), fp8=self.attention == 'fp8')
            att_i = att
            if i == c.n_layer - 1 and 0 < tail_views < V:
                # the last block: only the requested views' rows go on (their attention rows and residual rows, gathered; see prune_last_block)
                k = tail_views
                M = B * k * L
                att_i = att.view(B, V, L, d)[:, V - k:].reshape(M, d)
                h = h.view(B, V, L, d)[:, V - k:].reshape(M, d)
            h = self._gemm(att_i, p + '.attn.c_proj', M, res=h)
            m = ops.layernorm(h, *self._ln[p + '.ln_2'], M, d, out_bf16=act16)
            f = self._gemm(m, p + '.mlp.c_fc', M, epilogue=ops.EPI_GELU, out_bf16=act16)
            h = self._gemm(f, p + '.mlp.c_proj', M, res=h)
        if 0 < tail_views < V and c.n_layer == 0:
            h = h.view(B, V, L, d)[:, V - tail_views:].reshape(B * tail_views * L, d)
            M = B * tail_views * L
        return ops.layernorm(h, *self._ln['ln_f'], M, d)                    # migt.py:408

    # ------------------------------------------------------------------ many novel views from one context (prefix cache)
    def _check_render_shapes(self, L):
        c = self.config
        if self._sd_host is None or self.device is None:
            raise RuntimeError('MIGT: load_state_dict() and .to("cuda") first')
        if self.attention == 'fp8':
            raise ops._lib.VfError("the prefix-cache attention has a bf16 and an fp32-equivalent arm: attention='fp8' is not supported")
        if c.d_model // c.n_head != 64 or c.d_model % c.n_head or L != 64:
            raise ops._lib.VfError(f'prefix-cache attention supports head dim 64 and 64-token views only (got head dim '
                                   f'{c.d_model // c.n_head}, {L} tokens)')

    def prefill_context(self, codes, cameras, capacity=None, pack=None):
        """Run the C context views once and keep every layer's keys and values: ``codes`` int [B,C,t,t], ``cameras`` fp32 [B,C,7]
        (relative + normalised) -> ContextCache for ``generate_from_context``.  Block-causal attention never shows a context view the
        target, ``wpe`` indexes the token inside a view and the poses are relative to view 0, so the context's hidden states — and each
        layer's K / V for them — do not depend on the query.  The cache IS each layer's fused c_attn output (thirds V, Q, K; the Q
        third is not read again): no copy, dtype as the arm's ``qkv``.
        ``capacity`` >= C: room for that many views per scene and layer ([B*capacity*L, 3d], scenes capacity*L*3d apart), the prefilled
        views put there by ``ops.kv_append`` at position 0 — for ``append_to_context`` / ``rollout_from_context``, which otherwise
        reallocate at their first call.  Without it: the buffers and launches above, nothing else.
        ``pack``: None, or ``'kv'`` / ``'e4m3'`` (``'e4m3'``: ``precision='bf16'`` models only): fill a GROWING packed cache of that form
        directly — each layer's fused c_attn output goes to the packed buffers by that form's one append launch at
        position 0 and is dropped, so the plain cache of all layers never exists — with every tensor equal, bit for bit, to
        ``prefill_context(codes, cameras).pack(dtype, room=capacity - C)``."""
        if pack not in (None, 'kv', 'e4m3'):
            raise ValueError(f"prefill_context: pack None, 'kv' or 'e4m3' expected, got {pack!r}")
        if pack == 'e4m3' and self.precision != 'bf16':
            raise ValueError(f"prefill_context: pack='e4m3' is for precision='bf16' models; the {self.precision!r} arm exists for "
                             "exactness: pack='kv' keeps its bits")
        codes = torch.as_tensor(codes).to(self.device)
        cameras = torch.as_tensor(cameras, dtype=torch.float32).to(self.device)
        if codes.dim() < 3 or cameras.shape[:2] != codes.shape[:2] or cameras.shape[-1] != 7 or codes.shape[1] < 1:
            raise ValueError(f'prefill_context: codes [B,C,t,t] and cameras [B,C,7] expected, got {tuple(codes.shape)} and {tuple(cameras.shape)}')
        B, C = codes.shape[:2]
        if capacity is not None and (isinstance(capacity, bool) or int(capacity) != capacity or int(capacity) < C):
            raise ValueError(f'prefill_context: capacity, an integer >= C = {C}, expected, got {capacity}')
        tshape = tuple(codes.shape[2:])
        L = int(np.prod(tshape))
        self._check_render_shapes(L)
        if pack is not None:
            c, cap = self.config, C if capacity is None else int(capacity)
            dt = torch.bfloat16 if self._act_dtypes()[1] else torch.float32
            if pack == 'kv':
                cache = GrowingKVCache(self, [GrowingKVCache.buffers(B, cap, L, c.d_model, dt, self.device) for _ in range(c.n_layer)],
                                       B, C, tshape, cap)
            else:
                cache = GrowingE4M3Cache(self, [GrowingE4M3Cache.buffers(B, cap, c.n_head, self.device) for _ in range(c.n_layer)],
                                         B, C, tshape, cap)
            sink = PrefillSink(cache, C)
            self._blocks(codes, self._pose_embed(cameras), B, C, L, kv_sink=sink)
            sink.close()
            return cache
        kv = []
        self._blocks(codes, self._pose_embed(cameras), B, C, L, kv_sink=kv)
        cache = ContextCache(self, kv, B, C, tshape)
        if capacity is not None and int(capacity) > C:                     # (capacity = C is the tight cache: nothing to move)
            cache.reallocate(int(capacity))
        return cache

    def _context_lengths(self, cache, n_context, N):
        """``n_context`` of the ``*_from_context`` methods -> int32 device tensor [B*N] for ``_query_rows``, or None (None in, on a
        cache without slack and without lengths of its own: every view sees all C cached views, the path and the launches without the
        keyword; a cache with slack or lengths always takes the length route, and its default lengths are its own: the fixed-C entry
        would read unfilled rows).  An int, [B] (one length per scene) or [B,N] (one per query view) of integers in [0, the filled length
        of the scene]: the view sees that many leading context views and itself, which is the model's answer for that context (0: no
        context at all).  Host data preferred (a device tensor is brought to the host once, to validate it); anything else: ValueError,
        before any launch (``ContextCache.plan_lengths``).  A group of 4 (bf16) / 2 (f32) consecutive views costs what its longest
        member costs, and rows are not reordered here."""
        plan = cache.plan_lengths(n_context, N)
        return None if plan is None else torch.from_numpy(plan.reshape(-1)).to(self.device)

    def _query_rows(self, cache, ids32, add, N, n_context=None, append_at=None, tail='all', save=None):
        """The per-layer loop over the rows of N query views per scene of ``cache``: ``ids32`` int32 [B*N*L] token ids, ``add`` fp32
        [B*N, d] (a pose embedding or the LOC row per view) -> ln_f hidden states [B*N*L, d].  Each view attends to the cached context
        and to itself (ops.attn_prefix); its rows go through the LayerNorm / dense launches of the full pass.  ``n_context``: None, or an
        int32 device tensor [B*N] (``_context_lengths``): view (b, n) attends to the first ``n_context[b*N+n]`` cached views only — the
        model's answer for a context of that many views, since the first c views of a C-view cache are the cache of those c views.
        Rows are not reordered: the attention's workgroups take 4 (bf16) / 2 (f32) consecutive views, and a group costs what its
        longest member costs.
        ``append_at``: None, or an int32 device tensor [B]: in every layer, after c_attn, the keys and values of view n of scene b are put
        into the cache's view ``append_at[b] + n`` (ops.kv_append) BEFORE the attention, so that with ``n_context[b*N+n] = append_at[b] + n``
        view n attends to the old context, to the views 0 ... n-1 of this pass and to itself: block-causal attention, same kernel.
        ``tail``: 'all' (the hidden states of every row), a view number n (the last block's projection, MLP and ln_f on that view's
        rows only -> [B*L, d]; the rows that are returned keep their bits) or None (nothing is returned: the last block ends once its
        keys and values are in the cache).
        ``save``: None (the path and the launches without the keyword), or a list that receives what a backward pass over these rows
        needs (``score_grad_from_context``): per layer the tuple (the block's input h, the residual stream after the attention, the
        layer's fused c_attn output in a buffer of its own, the LayerNorm-2 output), then the final h that ``ln_f`` reads.  Same launches
        on the same values: the hidden states keep their bits.  With ``tail='all'`` only.
        The cache's form (plain, forked, packed) is the cache's own business: ``plan_pass`` refuses what the form cannot serve before
        any launch, ``append`` and ``attend`` issue the form's launch (viewformer_amd/context_cache.py)."""
        c, dev = self.config, self.device
        if save is not None and tail != 'all':
            raise ValueError('_query_rows: save goes with tail="all" (a backward pass needs every row)')
        B, L = cache.B, cache.L
        d, nE = c.d_model, c.n_embeddings
        M = B * N * L
        if append_at is not None and n_context is None:
            raise ValueError('_query_rows: appended views carry their context lengths')
        at = cache.plan_pass(n_context, append_at, save)
        h = ops.embed_sum(ids32, self._wte, self._wpe, add, B * N, L, d, nE + 2)           # migt.py:392
        act16, qkv16 = cache.act16, cache.qkv16
        att = torch.empty((M, d), dtype=torch.bfloat16 if act16 else torch.float32, device=dev)
        qkv = torch.empty((M, 3 * d), dtype=torch.bfloat16 if qkv16 else torch.float32, device=dev)
        for i in range(c.n_layer):                                           # Block.call on the query rows, migt.py:230-238
            p = f'h.{i}'
            last = i == c.n_layer - 1
            a = ops.layernorm(h, *self._ln[p + '.ln_1'], M, d, out_bf16=act16)
            if save is not None and i:
                qkv = torch.empty_like(qkv)                                  # the backward reads every layer's q / k / v again
            h_in = h
            self._dense_launch(a, self._dense[p + '.attn.c_attn'], M, qkv)
            if append_at is not None:
                cache.append(i, qkv, N, at)
            if last and tail is None:
                return None                                                  # the last block's other launches feed nothing: the keys and values are in
            cache.attend(i, qkv, att, N, n_context)
            att_i = att
            if last and tail != 'all' and N > 1:
                # the last block: only the returned view's rows go on (as _blocks' tail_views: the other views' rows feed nothing)
                M = B * L
                att_i = att.view(B, N, L, d)[:, tail].reshape(M, d)
                h = h.view(B, N, L, d)[:, tail].reshape(M, d)
            h = self._gemm(att_i, p + '.attn.c_proj', M, res=h)
            m = ops.layernorm(h, *self._ln[p + '.ln_2'], M, d, out_bf16=act16)
            if save is not None:
                save.append((h_in, h, qkv, m))
            f = self._gemm(m, p + '.mlp.c_fc', M, epilogue=ops.EPI_GELU, out_bf16=act16)
            h = self._gemm(f, p + '.mlp.c_proj', M, res=h)
        if save is not None:
            save.append(h)
        return ops.layernorm(h, *self._ln['ln_f'], M, d)                     # migt.py:408

    def _context_args(self, what, cache, cameras=None, codes=None, n_context=None, one_photo=False, needs=None, view0=None, lengths=True):
        """The front matter of every method that takes a cache, in ``score_from_context``'s order: the cache (a ContextCache that can do
        what ``needs`` — None, ``'room'`` or ``'backward'`` —, of a shape and arm with prefix-cache attention, of this model; ``'room'``
        lets a plain cache, a fork and a GROWING packed cache through, never a read-only packed one), the optional ``cameras`` fp32
        [B,N,7], the optional ``codes`` int [B,N,t,t] (``one_photo``: or [B,1,t,t]), sample's ``view0`` and ``n_context``
        -> (cameras and codes on the device, N, L, the context lengths as ``_context_lengths`` makes them, None without ``lengths``).
        Every refusal comes before any launch and before the one host-to-device copy of the lengths."""
        if not isinstance(cache, ContextCache):
            raise TypeError(f'{what}: a ContextCache from prefill_context expected')
        if needs is not None:
            (cache.refuse_backward if needs == 'backward' else cache.refuse_growth if needs == 'room' else cache.refuse_packed)(what)
        B, tshape, L = cache.B, cache.tshape, cache.L
        self._check_render_shapes(L)                                         # an arm or shape without prefix-cache attention: refused whatever the cache
        cache.check(self)
        N = None
        if cameras is not None:
            cameras = torch.as_tensor(cameras, dtype=torch.float32).to(self.device)
            if cameras.dim() != 3 or cameras.shape[0] != B or cameras.shape[2] != 7:
                raise ValueError(f'{what}: cameras [B={B},N,7] expected for this cache, got {tuple(cameras.shape)}')
            N = cameras.shape[1]
        if codes is not None:
            codes = torch.as_tensor(codes).to(self.device)
            if (codes.dim() != 2 + len(tshape) or codes.shape[0] != B or tuple(codes.shape[2:]) != tshape or codes.dtype.is_floating_point
                    or codes.dtype == torch.bool or not (N is None or codes.shape[1] == N or (one_photo and codes.shape[1] == 1))):
                raise ValueError(f'{what}: codes int [B={B},N={N}{" or 1" if one_photo else ""},{",".join(map(str, tshape))}] expected for this '
                                 f'cache, got {codes.dtype} {tuple(codes.shape)}')
            N = codes.shape[1] if N is None else N
        if view0 is not None and (view0 < 0 or (view0 + N) * L >= 1 << 32):
            raise ValueError(f'{what}: 0 <= view0 and (view0 + N) * {L} < 2^32 expected, got view0 = {view0}, N = {N}')
        return cameras, codes, N, L, self._context_lengths(cache, n_context, N) if lengths else None

    def _mask_rows(self, cameras, L):
        """N MASK views per scene at ``cameras`` [B,N,7] -> (``ids32``, ``add``) for ``_query_rows``: the MASK token on every row, the
        cameras' pose embedding per view"""
        B, N = cameras.shape[:2]
        add = self._pose_embed(cameras).contiguous().view(B * N, self.config.d_model)
        return torch.full((B * N * L,), self.mask_token, dtype=torch.int32, device=self.device), add

    @staticmethod
    def _sampler_args(what, n_samples, temperature, top_k, top_p):
        """the sampler's arguments as ``ops.sample_rows`` takes them, refused here before any launch -> n_samples as an int"""
        if not 1 <= int(n_samples) <= 65535 or int(n_samples) != n_samples:
            raise ValueError(f'{what}: 1 <= n_samples <= 65535 expected, got {n_samples}')
        if not (float(temperature) > 0 and math.isfinite(float(temperature))) or not float(top_p) > 0 or int(top_k) < 0:
            raise ValueError(f'{what}: temperature > 0 (finite), top_p > 0 and top_k >= 0 expected, got {temperature}, {top_p}, {top_k}')
        return int(n_samples)

    def generate_from_context(self, cache, query_cameras, codes_only: bool = True, return_confidence: bool = False, n_context=None):
        """N novel views per scene from a prefilled context: ``query_cameras`` fp32 [B,N,7] in the context's (relative, normalised)
        frame -> generated code maps int64 [B,N,t,t], or with ``codes_only=False`` the logits [B,N,t,t,n_embeddings].  Every query is
        a MASK view with its pose embedding — the last view of ``model(dict(input_ids=[ctx, MASK], poses=[ctx, query]))`` — whose
        rows go through the same LayerNorm / dense launches as there (on B*N*L rows) and whose attention reads the context's keys and
        values from the cache (ops.attn_prefix).  Queries are independent of each other: a query's rows do not depend on N.
        ``return_confidence`` (with ``codes_only``): (codes, confidence, entropy), the last two fp32 [B,N,t,t] — log p of the generated
        code (max logit - lse) and the entropy of the token's distribution, from the same LM-head launch (``_lm_score``).
        ``n_context``: how many leading context views each query sees (``_context_lengths``; None: all C, the launches without the
        keyword); consecutive views share an attention group, which costs what its longest member costs."""
        if return_confidence and not codes_only:
            raise ValueError('generate_from_context: return_confidence goes with codes_only=True (the logits say it all)')
        query_cameras, _, N, L, ctx = self._context_args('generate_from_context', cache, query_cameras, n_context=n_context)
        dev, nE, B, tshape = self.device, self.config.n_embeddings, cache.B, cache.tshape
        M = B * N * L
        if N == 0:
            if return_confidence:
                return (torch.empty((B, 0, *tshape), dtype=torch.int64, device=dev), torch.empty((B, 0, *tshape), dtype=torch.float32, device=dev),
                        torch.empty((B, 0, *tshape), dtype=torch.float32, device=dev))
            return (torch.empty((B, 0, *tshape), dtype=torch.int64, device=dev) if codes_only
                    else torch.empty((B, 0, *tshape, nE), dtype=torch.float32, device=dev))
        hf = self._query_rows(cache, *self._mask_rows(query_cameras, L), N, ctx)
        if return_confidence:
            st = self._lm_score(hf, M, want=('idx', 'max_logit', 'lse', 'entropy'))
            return st['idx'].view(B, N, *tshape), (st['max_logit'] - st['lse']).view(B, N, *tshape), st['entropy'].view(B, N, *tshape)
        gen = self._lm_argmax(hf, M) if codes_only else None
        if gen is None:
            lg = torch.empty((M, nE), dtype=torch.float32, device=dev)
            self._lm(hf, M, lg)                                              # migt.py:417
            if not codes_only:
                return lg.view(B, N, *tshape, nE)
            gen = ops.argmax_rows(lg, M, nE)
        return gen.view(B, N, *tshape)

    def score_from_context(self, cache, query_cameras, codes, fused: bool = False, n_context=None):
        """How well do photos fit cameras?  ``query_cameras`` fp32 [B,N,7] in the context's (relative, normalised) frame, ``codes`` int
        [B,N,t,t] (one photo per camera) or [B,1,t,t] (one photo per scene against N candidate cameras) -> dict of
            token_log_prob  fp32 [B,N,t,t]   log p(code) under the MASK view at that camera: target logit - lse
            log_likelihood  fp32 [B,N]       its sum over a view's tokens, in token order
            predicted_codes int64 [B,N,t,t]  what generate_from_context generates there
            confidence      fp32 [B,N,t,t]   log p of the predicted code: max logit - lse
            entropy         fp32 [B,N,t,t]   of the token's distribution (nats)
            accuracy        fp32 [B,N]       share of a view's tokens where the prediction is the photo's code
        Every camera is a MASK view exactly as in ``generate_from_context`` (same pose embedding, same ``_query_rows`` launches); the LM
        head then yields five numbers per row (``_lm_score``: through the logits and the row kernel; ``fused=True``: in the bf16 head's
        epilogue without the logits, the slower route on the MI355X, kept for A/B runs and tests).  A code outside [0, n_embeddings) has log-probability -inf.  Views are independent: a view's results do not depend on N.
        ``n_context``: how many leading context views each query sees (``_context_lengths``; None: all C, the launches without the
        keyword); consecutive views share an attention group, which costs what its longest member costs."""
        query_cameras, codes, N, L, ctx = self._context_args('score_from_context', cache, query_cameras, codes, n_context, one_photo=True)
        dev, B, tshape = self.device, cache.B, cache.tshape
        M = B * N * L
        if N == 0:
            e4 = lambda dt: torch.empty((B, 0, *tshape), dtype=dt, device=dev)
            e2 = lambda: torch.empty((B, 0), dtype=torch.float32, device=dev)
            return dict(token_log_prob=e4(torch.float32), log_likelihood=e2(), predicted_codes=e4(torch.int64), confidence=e4(torch.float32),
                        entropy=e4(torch.float32), accuracy=e2())
        target = codes.to(torch.int32).expand(B, N, *tshape).reshape(M).contiguous()
        hf = self._query_rows(cache, *self._mask_rows(query_cameras, L), N, ctx)
        st = self._lm_score(hf, M, target, fused=fused)
        tlp, conf, ll, acc = ops.score_views(st, target, B * N, L)           # log-likelihood: one fp32 chain per view, in token order
        return dict(token_log_prob=tlp.view(B, N, *tshape), log_likelihood=ll.view(B, N), predicted_codes=st['idx'].view(B, N, *tshape),
                    confidence=conf.view(B, N, *tshape), entropy=st['entropy'].view(B, N, *tshape), accuracy=acc.view(B, N))

    def match_from_context(self, cache, query_cameras, codes, n_context=None):
        """Which of M cameras does each of P photos belong to?  ``query_cameras`` fp32 [B,M,7] in the context's (relative, normalised)
        frame, ``codes`` int [B,P,t,t] or [1,P,t,t] (one photo set for all scenes) -> dict of
            log_likelihood  fp32 [B,P,M]     of photo p under the MASK view at camera m: what ``score_from_context(cache,
                                             query_cameras[:, m:m+1], codes[:, p:p+1])['log_likelihood'][:, 0]`` gives, bit for bit
            accuracy        fp32 [B,P,M]     share of photo p's tokens that view m predicts, likewise
            predicted_codes int64 [B,M,t,t], confidence fp32 [B,M,t,t], entropy fp32 [B,M,t,t]: of the cameras, as ``score_from_context``'s
        A scored view's logits depend on the context and the camera only, so the P x M matrix costs M query views (``_query_rows``, as
        ``score_from_context``: the cache's form stays the cache's business), one LM head over them with the logits written, the row
        kernel, and one gather-and-sum launch (``ops.match_views``) — never the fused head, which writes no logits.  ``log_likelihood``
        and ``accuracy`` are TRANSPOSED VIEWS of the kernel's camera-major [B,M,P] output (not contiguous); a code outside
        [0, n_embeddings) makes its photo's log-likelihood -inf.  M = 0: empty tensors, nothing is launched; P = 0: an empty matrix
        beside the cameras' own outputs, without the matching launch.  ``n_context``: as ``score_from_context``'s (an int, [B] or [B,M])."""
        what = 'match_from_context'
        query_cameras, _, M, L, _ = self._context_args(what, cache, query_cameras, lengths=False)
        dev, nE, B, tshape = self.device, self.config.n_embeddings, cache.B, cache.tshape
        codes = torch.as_tensor(codes).to(dev)
        if (codes.dim() != 2 + len(tshape) or codes.shape[0] not in (1, B) or tuple(codes.shape[2:]) != tshape or codes.dtype.is_floating_point
                or codes.dtype == torch.bool):
            raise ValueError(f'{what}: codes int [B={B} or 1,P,{",".join(map(str, tshape))}] expected for this cache, got {codes.dtype} '
                             f'{tuple(codes.shape)}')
        ctx = self._context_lengths(cache, n_context, M)
        P = codes.shape[1]
        R = B * M * L
        empty = lambda: torch.empty((B, M, P), dtype=torch.float32, device=dev).transpose(1, 2)
        if M == 0:                                                           # nothing is launched
            e4 = lambda dt: torch.empty((B, 0, *tshape), dtype=dt, device=dev)
            return dict(log_likelihood=empty(), accuracy=empty(), predicted_codes=e4(torch.int64), confidence=e4(torch.float32),
                        entropy=e4(torch.float32))
        hf = self._query_rows(cache, *self._mask_rows(query_cameras, L), M, ctx)
        lg = torch.empty((R, nE), dtype=torch.float32, device=dev)
        self._lm(hf, R, lg)                                                  # migt.py:417
        st = ops.logits_score(lg, R, nE, want=('idx', 'max_logit', 'lse', 'entropy'))
        if P == 0:                                                           # the cameras' own outputs; no photo, no matching launch
            ll, acc = empty(), empty()
        else:
            ll, acc = (x.transpose(1, 2) for x in ops.match_views(lg, st['lse'], st['idx'], codes.to(torch.int32).reshape(-1, P, L).contiguous(),
                                                                  B, M, P, L, nE))
        return dict(log_likelihood=ll, accuracy=acc, predicted_codes=st['idx'].view(B, M, *tshape),
                    confidence=(st['max_logit'] - st['lse']).view(B, M, *tshape), entropy=st['entropy'].view(B, M, *tshape))

    # ------------------------------------------------------------------ gradient of the score with respect to the query cameras
    def _dense_T(self, name):
        """the native-fp32 TRANSPOSED pack of a dense layer, for dx = dy @ W^T on ``ops.igemm`` (MIGTTrainer._linear_dx's last branch), made
        on first use and kept until the weights are replaced; ``'wte'``: ``wte[:n_embeddings]`` as an [n_embeddings -> d] layer, the
        transpose of the tied LM head"""
        dn = self._head if name == 'wte' else self._dense[name]
        if 'f32' not in dn.packed_T:
            w, sk, sn = (self._wte, dn.k, 1) if name == 'wte' else (dn.w_raw, 1, dn.n)          # (the head's weight lies transposed)
            dn.packed_T['f32'] = ops.pack(w, dn.n, dn.k, 1, sk=sk, sn=sn, st=0)
        return dn.packed_T['f32']

    def _linear_dx(self, name, dy, M, res=None):
        """dx [M, k] = dy [M, n] @ W^T (+ res) in native fp32, whatever the arm of the forward"""
        dn = self._head if name == 'wte' else self._dense[name]
        dx = torch.empty((M, dn.k), dtype=torch.float32, device=dy.device)
        ops.igemm(dy, self._dense_T(name), M, dn.n, dn.k, dx, res=res)
        return dx

    def _pose_embed_bwd(self, poses, dadd):
        """backward of ``_pose_embed``: ``dadd`` fp32 [B*N, d], the gradient of the pose embedding -> the gradient of ``poses`` [B,N,7]
        (the 7 numbers free).  c_proj^T, the exact-erf GELU's derivative at the recomputed pre-activation, c_fc^T (a layer with 7
        outputs: ``dense_small_n`` where its shape rule admits, else the native GEMM), then the pose multiplier on the position columns."""
        from . import train_ops as T
        B, Sp, _ = poses.shape
        c = self.config
        R = B * Sp
        fc = self._dense['pose_embedding.c_fc']
        pin = geometry.pose_model_input(poses, c.pose_multiplier).reshape(R, 7).contiguous()
        u = ops.dense_small_k(pin, fc.w_raw, fc.bias, R, 7, fc.n, gelu=False)
        du = T.gelu_bwd(u, self._linear_dx('pose_embedding.c_proj', dadd, R))
        if T.dense_small_n_supported(fc.n, fc.k):
            if fc.w_raw_T is None:
                fc.w_raw_T = T.transpose(fc.w_raw, fc.k, fc.n).view(fc.n, fc.k)
            dpin = T.dense_small_n(du, fc.w_raw_T, None, R, fc.n, fc.k)
        else:
            dpin = self._linear_dx('pose_embedding.c_fc', du, R)
        # (a Python scalar: a constant built on the host would be a blocking copy, and a synchronise, in every pass)
        return torch.cat([dpin[:, :3] * c.pose_multiplier, dpin[:, 3:]], -1).view(B, Sp, 7)

    def _score_backward(self, cache, poses, ids32, lg, target, saved, N, ctx):
        """d sum_tokens log p(code) / d poses [B,N,7] from what ``_query_rows(save=...)`` kept: every step a HIP launch of the training
        step's kernels in fp32 (train_ops.py), the attention's by ``ops.attn_prefix_bwd``.  The cache is a constant of the query camera
        (DESIGN.md §6.16), so the gradient stops there; weight gradients go to scratch and are dropped."""
        from . import train_ops as T
        c, dev = self.config, self.device
        B, L = cache.B, cache.L
        d, nE = c.d_model, c.n_embeddings
        M = B * N * L
        dgam, dbet = torch.empty(d, dtype=torch.float32, device=dev), torch.empty(d, dtype=torch.float32, device=dev)
        # + log-likelihood: dlogits = onehot - softmax = (softmax - onehot) * (-1).  A code outside [0, n_embeddings) has log-probability
        # -inf and no gradient: its row gets weight 0 (and a target inside the row, which the kernel reads)
        valid = (target >= 0) & (target < nE)
        w = torch.where(valid, -1.0, 0.0).to(torch.float32)
        _, dlg = T.softmax_ce(lg, target.clamp(0, nE - 1), w, M, nE)
        dh = self._linear_dx('wte', dlg, M)
        dh = T.layernorm_bwd(dh, saved[-1], self._ln['ln_f'][0], dgam, dbet, M, d, accumulate=False)
        for i in reversed(range(c.n_layer)):
            p = f'h.{i}'
            h_in, h_mid, qkv, m = saved[i]
            df = self._linear_dx(p + '.mlp.c_proj', dh, M)
            u = self._gemm(m, p + '.mlp.c_fc', M)                            # the pre-activation again, without the GELU epilogue
            dm = self._linear_dx(p + '.mlp.c_fc', T.gelu_bwd(u, df), M)
            dh = T.layernorm_bwd(dm, h_mid, self._ln[p + '.ln_2'][0], dgam, dbet, M, d, accumulate=False, res=dh)
            datt = self._linear_dx(p + '.attn.c_proj', dh, M)
            dqkv = torch.empty((M, 3 * d), dtype=torch.float32, device=dev)
            cache.attend_backward(i, qkv, datt, dqkv, N, ctx)
            da = self._linear_dx(p + '.attn.c_attn', dqkv, M)
            dh = T.layernorm_bwd(da, h_in, self._ln[p + '.ln_1'][0], dgam, dbet, M, d, accumulate=False, res=dh)
        dwte = torch.empty((nE + 2, d), dtype=torch.float32, device=dev)
        dwpe = torch.empty_like(self._wpe)
        dadd = T.embed_bwd(dh, ids32, dwte, dwpe, B * N, L, d, nE + 2)
        return self._pose_embed_bwd(poses, dadd)

    def score_grad_from_context(self, cache, query_cameras, codes, n_context=None):
        """``score_from_context`` (through the logits: its ``fused=False`` route, the same launches, every key with the same bits) plus
            grad_cameras  fp32 [B,N,7]   d log_likelihood[b,n] / d query_cameras[b,n], the 7 numbers treated as free
        — which way each camera should move so that its photo fits better.  One backward pass over the query rows in fp32 on both
        arms (``_score_backward``); the cached context is a constant of the query camera, so nothing flows into the cache.  The
        gradient of a view depends on that view alone.  A code outside [0, n_embeddings) (log-probability -inf) contributes no
        gradient.  ``n_context``: as ``score_from_context``'s."""
        query_cameras, codes, N, ctx = self._score_grad_args('score_grad_from_context', cache, query_cameras, codes, n_context)
        return self._score_grad(cache, query_cameras, codes, N, ctx)

    def _score_grad_args(self, what, cache, query_cameras, codes, n_context):
        """``score_from_context``'s validation, in its order -> (cameras and codes on the device, N, the context lengths as
        ``_context_lengths`` makes them: None or an int32 device tensor [B*N], planned on the host and copied once)"""
        query_cameras, codes, N, _, ctx = self._context_args(what, cache, query_cameras, codes, n_context, one_photo=True, needs='backward')
        return query_cameras, codes, N, ctx

    def _score_grad(self, cache, query_cameras, codes, N, ctx):
        """``score_grad_from_context`` on validated device tensors and prepared context lengths: launches only, nothing here waits for
        the device or copies from the host (tests/test_hip_score_grad.py runs it under torch's synchronisation check)"""
        dev, nE, B, tshape, L = self.device, self.config.n_embeddings, cache.B, cache.tshape, cache.L
        M = B * N * L
        if N == 0:
            res = self.score_from_context(cache, query_cameras, codes)
            res['grad_cameras'] = torch.empty((B, 0, 7), dtype=torch.float32, device=dev)
            return res
        target = codes.to(torch.int32).expand(B, N, *tshape).reshape(M).contiguous()
        ids32, add = self._mask_rows(query_cameras, L)
        saved = []
        hf = self._query_rows(cache, ids32, add, N, ctx, save=saved)
        lg = torch.empty((M, nE), dtype=torch.float32, device=dev)
        self._lm(hf, M, lg)                                                  # migt.py:417
        st = ops.logits_score(lg, M, nE, target=target)
        tlp, conf, ll, acc = ops.score_views(st, target, B * N, L)
        grad = self._score_backward(cache, query_cameras, ids32, lg, target, saved, N, ctx)
        return dict(token_log_prob=tlp.view(B, N, *tshape), log_likelihood=ll.view(B, N), predicted_codes=st['idx'].view(B, N, *tshape),
                    confidence=conf.view(B, N, *tshape), entropy=st['entropy'].view(B, N, *tshape), accuracy=acc.view(B, N),
                    grad_cameras=grad)

    def refine_from_context(self, cache, cameras0, codes, steps: int = 16, step_xyz: float = 0.05, step_rot: float = 0.05, n_context=None,
                            return_trace: bool = False):
        """Move cameras so that their photos fit better: a monotone gradient ascent on ``log_likelihood`` per view, from ``cameras0``
        fp32 [B,N,7] (the cache's frame, scored as they are given) with ``codes`` as ``score_from_context`` takes them.
        Every step proposes ``render.ascend_poses(p, g, s_xyz, s_rot)`` for all views — a step of length s_xyz along the position
        gradient and of s_rot along the tangent part of the quaternion gradient — and scores the candidates in ONE
        ``score_grad_from_context`` pass; a view whose log-likelihood rose takes its candidate and the gradient there, every other view
        keeps its camera and gradient and halves both of its steps.  Arguments are validated, brought to the device and (``n_context``, or a
        cache with slack or lengths of its own) turned into a device tensor of context lengths ONCE, before the first pass; after that
        nothing synchronises with the host or copies from it: the steps are enqueued back to back.  ``step_xyz`` / ``step_rot`` are
        starting values that the halving adapts.  A view whose log-likelihood at ``cameras0`` is -inf (a code outside [0, n_embeddings))
        or NaN never takes a candidate (-inf > -inf is false): it keeps ``cameras0`` and only halves its steps.  -> dict of
            cameras                 fp32  [B,N,7]  the refined cameras, in the cache's frame
            log_likelihood          fp32  [B,N]    there: never below ...
            initial_log_likelihood  fp32  [B,N]    ... the one at ``cameras0``
            accepted                int32 [B,N]    how many of the ``steps`` proposals each view took
        and with ``return_trace`` ``trace`` fp32 [steps+1,B,N], the log-likelihood after every step (non-decreasing)."""
        from .render import ascend_poses
        if not isinstance(cache, ContextCache):
            raise TypeError('refine_from_context: a ContextCache from prefill_context expected')
        if isinstance(steps, bool) or int(steps) != steps or int(steps) < 0:
            raise ValueError(f'refine_from_context: steps, an integer >= 0, expected, got {steps}')
        if not (float(step_xyz) > 0 and float(step_rot) > 0 and math.isfinite(float(step_xyz)) and math.isfinite(float(step_rot))):
            raise ValueError(f'refine_from_context: positive finite step_xyz and step_rot expected, got {step_xyz} and {step_rot}')
        B = cache.B
        p, codes, N, ctx = self._score_grad_args('refine_from_context', cache, cameras0, codes, n_context)
        r = self._score_grad(cache, p, codes, N, ctx)
        ll, g = r['log_likelihood'], r['grad_cameras']
        ll0 = ll.clone()
        s_xyz = torch.full((B, N), float(step_xyz), dtype=torch.float32, device=self.device)
        s_rot = torch.full((B, N), float(step_rot), dtype=torch.float32, device=self.device)
        accepted = torch.zeros((B, N), dtype=torch.int32, device=self.device)
        trace = [ll]
        for _ in range(int(steps) if N else 0):
            cand = ascend_poses(p, g, s_xyz, s_rot)
            rc = self._score_grad(cache, cand, codes, N, ctx)
            up = rc['log_likelihood'] > ll                                   # (a NaN never wins)
            up7 = up.unsqueeze(-1)
            p, g = torch.where(up7, cand, p), torch.where(up7, rc['grad_cameras'], g)
            ll = torch.where(up, rc['log_likelihood'], ll)
            s_xyz, s_rot = torch.where(up, s_xyz, s_xyz * 0.5), torch.where(up, s_rot, s_rot * 0.5)
            accepted = accepted + up.to(torch.int32)
            trace.append(ll)
        res = dict(cameras=p, log_likelihood=ll, initial_log_likelihood=ll0, accepted=accepted)
        if return_trace:
            res['trace'] = torch.stack(trace + [ll] * (int(steps) + 1 - len(trace)), 0)
        return res

    def sample_from_context(self, cache, query_cameras, n_samples: int = 1, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                            seed: int = 0, view0: int = 0, return_logits: bool = False, n_context=None):
        """Draw S = ``n_samples`` code maps per query view from the model's distribution: ``query_cameras`` fp32 [B,N,7] in the context's
        (relative, normalised) frame -> dict of
            codes           int64 [B,N,S,t,t]  the draws
            token_log_prob  fp32  [B,N,S,t,t]  log p of each drawn code under the distribution it was drawn from (after the filters)
            log_likelihood  fp32  [B,N,S]      its sum over a view's tokens, in token order
            kept            int32 [B,N,t,t]    the size of the set each token was drawn from
        (``return_logits`` adds logits fp32 [B,N,t,t,n_embeddings]).  A MASK view's tokens are predicted in one pass and are independent
        of each other given the context, so the S samples share ONE transformer view and one set of logits — the bits of
        ``generate_from_context(codes_only=False)``: same pose embedding, ``_query_rows`` and ``_lm`` launches — followed by one row
        kernel (ops.sample_rows: temperature, top-k, top-p and the S Gumbel-max draws).  ``top_k = 1`` gives ``generate_from_context``'s
        codes whatever the seed.  The noise of token l of view n of scene b is keyed by (seed, row_id = (b << 32) | ((view0 + n) L + l),
        sample index), b being the scene's number in the cache's batch: a token's draws do not depend on B, on N or on how the views are chunked (``view0`` = the number of the chunk's
        first view).
        ``n_context``: how many leading context views each query sees (``_context_lengths``; None: all C, the launches without the
        keyword); consecutive views share an attention group, which costs what its longest member costs."""
        S, view0 = self._sampler_args('sample_from_context', n_samples, temperature, top_k, top_p), int(view0)
        query_cameras, _, N, L, ctx = self._context_args('sample_from_context', cache, query_cameras, n_context=n_context, view0=view0)
        dev, nE, B, tshape = self.device, self.config.n_embeddings, cache.B, cache.tshape
        M = B * N * L
        if N == 0:
            res = dict(codes=torch.empty((B, 0, S, *tshape), dtype=torch.int64, device=dev),
                       token_log_prob=torch.empty((B, 0, S, *tshape), dtype=torch.float32, device=dev),
                       log_likelihood=torch.empty((B, 0, S), dtype=torch.float32, device=dev),
                       kept=torch.empty((B, 0, *tshape), dtype=torch.int32, device=dev))
            if return_logits:
                res['logits'] = torch.empty((B, 0, *tshape, nE), dtype=torch.float32, device=dev)
            return res
        hf = self._query_rows(cache, *self._mask_rows(query_cameras, L), N, ctx)
        lg = torch.empty((M, nE), dtype=torch.float32, device=dev)
        self._lm(hf, M, lg)                                                  # migt.py:417
        row_id = ((torch.arange(B, dtype=torch.int64, device=dev) << 32).view(B, 1)
                  + (torch.arange(N * L, dtype=torch.int64, device=dev) + view0 * L).view(1, N * L)).reshape(M).contiguous()
        st = ops.sample_rows(lg, M, nE, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, row_id=row_id, n_samples=S,
                             want=('idx', 'logp', 'kept'))
        ll = ops.sample_views(st['logp'], B * N, L, S)                      # one fp32 chain per (view, sample), in token order
        res = dict(codes=st['idx'].view(B, N, L, S).permute(0, 1, 3, 2).reshape(B, N, S, *tshape),
                   token_log_prob=st['logp'].view(B, N, L, S).permute(0, 1, 3, 2).reshape(B, N, S, *tshape),
                   log_likelihood=ll.view(B, N, S), kept=st['kept'].view(B, N, *tshape))
        if return_logits:
            res['logits'] = lg.view(B, N, *tshape, nE)
        return res

    def expect_from_context(self, cache, query_cameras, embedding, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, n_context=None):
        """The EXPECTED view per query camera, in the codebook's latent space: ``query_cameras`` fp32 [B,N,7] in the context's (relative,
        normalised) frame and ``embedding`` fp32 [D, n_embeddings] on the device (``VQGAN.codebook_embedding()``) -> dict of
            latents  fp32  [B,N,t,t,D]  sum over the kept codes of p_n embedding[:, n] per token
            kept     int32 [B,N,t,t]    the size of the set each token's mean runs over
        A MASK view's tokens are independent given the context, so the mean of the distribution ``sample_from_context`` draws from (same
        ``temperature``, ``top_k``, ``top_p``) is known per token in closed form.  The launches are
        ``generate_from_context(codes_only=False)``'s — same pose embedding, ``_query_rows`` and ``_lm`` — followed by one row kernel
        (ops.mix_rows).  ``top_k = 1`` gives the embedding of ``generate_from_context``'s codes, bit for bit, on every token with a unique
        maximum.  There is no fallback: a shape the kernel does not take is refused.
        ``n_context``: how many leading context views each query sees (``_context_lengths``; None: all C, the launches without the
        keyword); consecutive views share an attention group, which costs what its longest member costs."""
        if isinstance(top_k, bool) or int(top_k) != top_k:
            raise ValueError(f'expect_from_context: an integer top_k expected, got {top_k}')
        self._sampler_args('expect_from_context', 1, temperature, top_k, top_p)
        nE = self.config.n_embeddings
        if (not torch.is_tensor(embedding) or embedding.dim() != 2 or embedding.dtype != torch.float32 or embedding.shape[1] != nE
                or not embedding.is_contiguous()):
            raise ValueError(f'expect_from_context: embedding fp32 [D, n_embeddings={nE}] (contiguous) expected, got '
                             f'{tuple(embedding.shape) if torch.is_tensor(embedding) else type(embedding).__name__}')
        own = self.device
        if own is not None and (embedding.device.type != own.type or (own.index is not None and embedding.device.index != own.index)):
            raise ValueError(f"expect_from_context: the embedding lives on {embedding.device}, the model on {self.device}")
        D = embedding.shape[0]
        if not ops.mix_rows_supported(D, nE):
            raise ValueError(f'expect_from_context: no mix kernel for D = {D}, n_embeddings = {nE} (D % 32 == 0, D <= 256, n_embeddings <= 1024)')
        query_cameras, _, N, L, ctx = self._context_args('expect_from_context', cache, query_cameras, n_context=n_context)
        dev, B, tshape = self.device, cache.B, cache.tshape
        M = B * N * L
        if N == 0:
            return dict(latents=torch.empty((B, 0, *tshape, D), dtype=torch.float32, device=dev),
                        kept=torch.empty((B, 0, *tshape), dtype=torch.int32, device=dev))
        hf = self._query_rows(cache, *self._mask_rows(query_cameras, L), N, ctx)
        lg = torch.empty((M, nE), dtype=torch.float32, device=dev)
        self._lm(hf, M, lg)                                                  # migt.py:417
        st = ops.mix_rows(lg, M, nE, embedding, D, temperature=temperature, top_k=top_k, top_p=top_p, want=('out', 'kept'))
        return dict(latents=st['out'].view(B, N, *tshape, D), kept=st['kept'].view(B, N, *tshape))

    def localize_from_context(self, cache, codes, return_tokens: bool = False, fused_tail: bool = True, n_context=None):
        """Localize N photos per scene against a prefilled context: ``codes`` int [B,N,t,t] (the photos' code maps) -> cameras fp32
        [B,N,7] in the context's (relative, normalised) frame; with ``return_tokens`` a dict(cameras, pose_prediction [B,N,L,7],
        raw [B,N,L,7] — the pose classifier's output before post-processing).  Every photo is a LOC view — ``wte[codes] + wpe +
        wte[LOC]``, no pose: the last view of ``model(dict(input_ids=[ctx, photo], poses=ctx_poses))`` — that sees the context and itself,
        which is ``generate_from_context``'s visibility: the same loop over its rows (``_query_rows``), no LM head, then the pose
        classifier.  ``fused_tail``: c_proj, the per-token post-processing and the reduction over a view's tokens as one launch
        (ops.pose_tail) where the kernel takes the shape; otherwise, and with ``fused_tail=False``, the GEMM and
        geometry.pose_head_postprocess / reduce_cameras as ``__call__`` and the evaluators run them.  Photos are independent of each
        other: a photo's result does not depend on N.
        ``n_context``: how many leading context views each query sees (``_context_lengths``; None: all C, the launches without the
        keyword); consecutive views share an attention group, which costs what its longest member costs."""
        if not self.use_localization:
            raise RuntimeError('localize_from_context needs a model with the localization head')
        _, codes, N, L, ctx = self._context_args('localize_from_context', cache, codes=codes, n_context=n_context)
        c, dev, d, B = self.config, self.device, self.config.d_model, cache.B
        M = B * N * L
        if N == 0:
            cams = torch.empty((B, 0, 7), dtype=torch.float32, device=dev)
            if not return_tokens:
                return cams
            return dict(cameras=cams, pose_prediction=torch.empty((B, 0, L, 7), dtype=torch.float32, device=dev),
                        raw=torch.empty((B, 0, L, 7), dtype=torch.float32, device=dev))
        add = self._wte[self.localization_token].view(1, d).expand(B * N, d).contiguous()            # migt.py:387-390
        ids32 = codes.reshape(M).to(torch.int32).contiguous()
        hf = self._query_rows(cache, ids32, add, N, ctx)
        p1 = self._gemm(hf, 'pose_criterion.pose_classifier.c_fc', M, epilogue=ops.EPI_GELU)
        cp = self._dense['pose_criterion.pose_classifier.c_proj']
        if fused_tail and cp.n == 7 and ops.pose_tail_supported(cp.k, L):
            cams, tokens, raw = ops.pose_tail(p1, cp.w_raw, cp.bias, c.pose_multiplier, B * N, L, want_raw=return_tokens,
                                              want_tokens=return_tokens)
        else:
            raw = self._gemm(p1, 'pose_criterion.pose_classifier.c_proj', M).view(B * N, L, 7)
            tokens = geometry.pose_head_postprocess(raw, c.pose_multiplier)
            cams = geometry.reduce_cameras(tokens, -2)
        cams = cams.view(B, N, 7)
        if not return_tokens:
            return cams
        return dict(cameras=cams, pose_prediction=tokens.view(B, N, L, 7), raw=raw.view(B, N, L, 7))

    # ------------------------------------------------------------------ a context that grows: appended views, roll-outs along a path
    def append_to_context(self, cache, codes, cameras):
        """Grow a context in place by K views per scene: ``codes`` int [B,K,t,t], ``cameras`` fp32 [B,K,7] in the context's (relative,
        normalised) frame -> the same ContextCache, K views longer in every scene.  ONE pass over the B*K*L new rows: a context view's own
        embedding (wte[codes] + wpe + pose embedding), and in every layer c_attn, ``ops.kv_append`` at each scene's own length, then
        ``ops.attn_prefix`` with ``ctx_len = length_b + j`` for new view j — which therefore attends to the old context, to the new views
        0 ... j-1 (in the cache at this layer already) and to itself: block-causal attention.  The first c views of a cache are the cache
        of those c views, so no earlier view is touched, and the grown cache holds what ``prefill_context`` of all views would within the
        arm's own error (the same row launches; the prefill's attention is the block-causal kernel, a new view's the prefix kernel).
        K views at once and one by one give the same bits where the dense layers take one kernel for both row counts.  Beyond the capacity the cache moves to
        buffers of max(2 capacity, needed) views, inside the same object.  Foreign caches, the fp8 arm and wrong shapes are refused
        before any launch."""
        cameras, codes, K, L, _ = self._context_args('append_to_context', cache, cameras, codes, needs='room', lengths=False)
        dev, d, B = self.device, self.config.d_model, cache.B
        if K == 0:
            return cache
        lengths = cache.filled()
        cache.reserve(int(lengths.max()) + K)
        pos = torch.from_numpy(lengths).to(dev)
        ctx = torch.from_numpy((lengths.reshape(B, 1) + np.arange(K, dtype=np.int32).reshape(1, K)).astype(np.int32).reshape(-1)).to(dev)
        add = self._pose_embed(cameras).contiguous().view(B * K, d)
        ids32 = codes.reshape(B * K * L).to(torch.int32).contiguous()
        self._query_rows(cache, ids32, add, K, ctx, append_at=pos, tail=None)
        cache.grown(lengths, K)
        return cache

    def _replicate(self, cache, S):
        return cache.replicate(S)

    # ------------------------------------------------------------------ forks: children that share a cache's views and own what they add
    def adopt_from_fork(self, parent, child, which, score=None):
        """Keep one child's trajectory: the own views of child ``which[b]`` of every scene b are appended to ``parent`` — one
        ``ops.kv_append`` per layer on a gathered source, no row is run again — which then holds what ``append_to_context`` of those views
        would have left (the child computed them against the parent's views and its own earlier ones: the same launches).  ``which``: int
        [B] (host or device) in [0, S), or ``'best'`` with ``score`` [B,S] (or [B,S,T], summed over T in order): the child with the
        largest score, ties going to the lowest index (``render.choose_best``).  Refused: a child of another cache, and a parent whose
        lengths have moved since the fork.  ``parent`` grows in place by the children's number of own views.  -> the adopted child per
        scene, int64 [B] (host)."""
        from .render import choose_best, plan_fork_lengths
        if not isinstance(parent, ContextCache) or not isinstance(child, ContextCache):
            raise TypeError('adopt_from_fork: two ContextCaches expected')
        parent.refuse_packed('adopt_from_fork')
        child.refuse_packed('adopt_from_fork')
        if not child.forked() or parent.forked():
            raise ValueError('adopt_from_fork: a plain parent cache and a cache forked from it expected')
        if child._parent is None or child._parent() is not parent:
            raise ValueError('adopt_from_fork: the child was not forked from this parent')
        parent.check(self)
        child.check(self)
        S, B = child.share, parent.B
        lengths = parent.filled()
        if child.B != B * S or not np.array_equal(np.repeat(lengths, S), child.split):
            raise ValueError(f'adopt_from_fork: the parent has grown since the fork (lengths {lengths.tolist()}, forked at '
                             f'{child.split[::S].tolist()}): fork again')
        if isinstance(which, str):
            if which != 'best' or score is None:
                raise ValueError("adopt_from_fork: which = 'best' goes with score [B,S]")
            sc = score.detach().float().cpu().numpy() if isinstance(score, torch.Tensor) else np.asarray(score, dtype=np.float32)
            if sc.ndim == 3:
                tot = np.zeros(sc.shape[:2], dtype=np.float32)
                for t in range(sc.shape[2]):                                 # in order, in fp32
                    tot = tot + sc[:, :, t]
                sc = tot
            if sc.shape != (B, S):
                raise ValueError(f'adopt_from_fork: score [B={B},S={S}] expected, got {sc.shape}')
            which = choose_best(sc)
        else:
            if score is not None:
                raise ValueError("adopt_from_fork: score goes with which = 'best'")
            which = np.asarray(which.detach().cpu().numpy() if isinstance(which, torch.Tensor) else which)
            if which.shape != (B,) or which.dtype == np.bool_ or not np.issubdtype(which.dtype, np.integer) or (
                    which.size and (which.min() < 0 or which.max() >= S)):
                raise ValueError(f'adopt_from_fork: which, integers [B={B}] in [0, S={S}), expected, got {which}')
        own = plan_fork_lengths(child.split, child.filled(), child.room)
        K = int(own[0]) if own.size else 0
        which = which.astype(np.int64)
        if K == 0:
            return which
        d, L, dev = self.config.d_model, parent.L, self.device
        parent.reserve(int(lengths.max()) + K)
        pos = torch.from_numpy(lengths).to(dev)
        idx = torch.from_numpy(np.arange(B, dtype=np.int64) * S + which).to(dev)
        for i, own_kv in enumerate(child.kv):
            parent.append(i, own_kv.view(B * S, child.room * L, 3 * d)[idx, :K * L].reshape(B * K * L, 3 * d), K, pos)
        parent.grown(lengths, K)
        return which

    def rollout_from_context(self, cache, path_cameras, n_samples: int = 1, temperature: float = 1.0, top_k: int = 1, top_p: float = 1.0,
                             seed: int = 0, return_logits: bool = False, fused_step: bool = True, fork: bool = False):
        """A camera path whose frames agree with each other: ``path_cameras`` fp32 [B,T,7] in the context's (relative, normalised) frame.
        For t = 0 ... T-1 view t is generated from the cache as it stands — the photographs AND the views 0 ... t-1 — and the generated
        code map is appended with camera t: by definition the loop ``sample_from_context`` of 1 view (``view0 = t``), then
        ``append_to_context``.  Codes are fed back on the device: no host synchronisation and no decode inside the loop.  -> dict of
            codes           int64 [B,S,T,t,t]
            token_log_prob  fp32  [B,S,T,t,t]  log p of each drawn code under the distribution it was drawn from (after the filters)
            log_likelihood  fp32  [B,S,T]      its sum over a view's tokens, in token order
            cache           the grown cache (T views longer; with S > 1 a replicated one of B*S scenes, ``cache`` itself untouched)
        (``return_logits`` adds logits fp32 [B,S,T,t,t,n_embeddings]).  ``fused_step`` (default): one pass per step over 2 views per
        scene — the append view of step t-1 and the MASK view of step t, ``ctx_len = (p, p+1)`` — with the last block's tail, ln_f and the
        LM head on the MASK rows only, and a trailing append pass after step T-1; the MASK view's keys land in the cache's next free
        view, beyond every length, where the next step's append view overwrites them.  ``fused_step=False``: the two passes of the
        definition.  Both give the definition's bits where the dense layers take one kernel for both row counts.
        ``top_k = 1`` (default) is the arg-max roll-out whatever the seed.  ``n_samples`` = S > 1: S independent trajectories per scene on
        a cache replicated to B*S scenes (scene b's copies at b*S ... b*S+S-1); the noise of token l of step t of trajectory (b, s) is
        keyed as ``sample_from_context`` keys scene b*S+s, view t, sample 0 — reproducible, and a prefix of a longer roll-out.
        ``fork=True`` (with S > 1; opt-in): the S trajectories run on ``cache.fork(S, room=T)`` instead of a replicated cache — the
        photographs' keys are read where they lie, only the T generated views per trajectory get buffers — with the same bits, the same
        noise keys and the fork as the returned ``cache`` (``adopt_from_fork`` keeps one trajectory in ``cache``)."""
        S = self._sampler_args('rollout_from_context', n_samples, temperature, top_k, top_p)
        path_cameras, _, T, L, _ = self._context_args('rollout_from_context', cache, path_cameras, needs='room', lengths=False)
        if fork:
            cache.refuse_packed('rollout_from_context(fork=True)')           # (a growing packed cache grows, but it is no fork's parent)
        c, dev = self.config, self.device
        d, nE, tshape, B = c.d_model, c.n_embeddings, cache.tshape, cache.B
        if T * L >= 1 << 32 or B * S >= 1 << 31:
            raise ValueError(f'rollout_from_context: T * {L} < 2^32 and B * n_samples < 2^31 expected, got T = {T}, B = {B}, n_samples = {S}')
        from .render import plan_rollout_lengths, plan_replication, rollout_row_ids
        if S > 1:                                                            # (fork=True on a fork: refused there, a fork of a fork)
            cache = cache.fork(S, T) if fork else cache.replicate(S)
            path_cameras = path_cameras[torch.from_numpy(plan_replication(B, S)).to(dev)]
        Bs = B * S
        M = Bs * L
        lengths = cache.filled()
        gen, pair = plan_rollout_lengths(lengths, T)                         # [T,Bs] and [T,Bs,2], host
        codes, tlps, lls, lgs = [], [], [], []
        if T:
            cache.reserve(int(lengths.max()) + T)
            gen_dev = torch.from_numpy(gen).to(dev)
            pair_dev = torch.from_numpy(pair.reshape(T, Bs * 2)).to(dev)
            pe = self._pose_embed(path_cameras)                              # [Bs,T,d]
            row0 = torch.from_numpy(rollout_row_ids(Bs, 0, L)).to(dev)
            mask_ids = torch.full((M,), self.mask_token, dtype=torch.int32, device=dev)
            prev = None
            for t in range(T):
                if t == 0 or not fused_step:
                    if t:
                        self._query_rows(cache, prev, pe[:, t - 1].contiguous(), 1, gen_dev[t - 1], append_at=gen_dev[t - 1], tail=None)
                    hf = self._query_rows(cache, mask_ids, pe[:, t].contiguous(), 1, gen_dev[t])
                else:
                    ids = torch.stack([prev.view(Bs, L), mask_ids.view(Bs, L)], 1).reshape(2 * M)
                    hf = self._query_rows(cache, ids, pe[:, t - 1:t + 1].reshape(Bs * 2, d), 2, pair_dev[t], append_at=gen_dev[t - 1], tail=1)
                lg = torch.empty((M, nE), dtype=torch.float32, device=dev)
                self._lm(hf, M, lg)                                          # migt.py:417
                st = ops.sample_rows(lg, M, nE, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, row_id=row0 + t * L, n_samples=1,
                                     want=('idx', 'logp'))
                lls.append(ops.sample_views(st['logp'], Bs, L, 1).view(Bs))  # one fp32 chain per view, in token order
                prev = st['idx'].view(M).to(torch.int32)
                codes.append(st['idx'].view(Bs, L)); tlps.append(st['logp'].view(Bs, L))
                if return_logits:
                    lgs.append(lg.view(Bs, L, nE))
            self._query_rows(cache, prev, pe[:, T - 1].contiguous(), 1, gen_dev[T - 1], append_at=gen_dev[T - 1], tail=None)
            cache.grown(lengths, T)
        stack = lambda xs, dt, *tail: (torch.stack(xs, 1) if xs else torch.empty((Bs, 0, *tail), dtype=dt, device=dev))
        res = dict(codes=stack(codes, torch.int64, L).view(B, S, T, *tshape), token_log_prob=stack(tlps, torch.float32, L).view(B, S, T, *tshape),
                   log_likelihood=stack(lls, torch.float32).view(B, S, T), cache=cache)
        if return_logits:
            res['logits'] = stack(lgs, torch.float32, L, nE).view(B, S, T, *tshape, nE)
        return res

    def generate_and_localize(self, codes, cameras, codes_only: bool = False):
        """The evaluator's two transformer passes (evaluate_transformer.py:119-123 and :134-136) as ONE pass.

        Pass 1 feeds [codes[:, :-1], MASK] with all S poses; pass 2 feeds all S real code maps with S-1 poses
        and the LOC embedding on the last view.  Views 0..S-2 are identical inputs in both, and block-causal
        attention never lets them see the last view, so their hidden states are bit-identical: only the last
        view differs.  We run S+1 views [ctx_0..ctx_{S-2}, MASK-view, LOC-view] with the last two marked as
        twins (each attends to the context and itself, never to its sibling) — the reference's own branch-stream
        construction (migt.py:392-401, branching_attention.py:94-125).  Every produced row equals the two-pass
        row bit-for-bit (tests/test_hip_models.py), at 8/14 of the transformer work for S = 7.

        codes [B,S,t,t] int (all S views encoded), cameras [B,S,7] float32 (relative + normalised).
        Returns (logits_last [B,t,t,n_embeddings], pose_prediction_last [B,1,L,7]); with ``codes_only`` the first member is the
        generated code map [B,t,t] int64 instead (arg-max fused into the LM head where the arm supports it)."""
        if not self.use_localization:
            raise RuntimeError('generate_and_localize needs a model with the localization head')
        c, dev = self.config, self.device
        codes = codes.to(dev)
        cameras = cameras.to(dev)
        B, S = codes.shape[:2]
        tshape = tuple(codes.shape[2:])
        L = int(np.prod(tshape))
        d, nE = c.d_model, c.n_embeddings
        if d // c.n_head != 64:
            raise ops._lib.VfError('attention kernel supports head dim 64 only')
        pose_emb = self._pose_embed(cameras)                                            # [B,S,d]
        lpe = self._wte[self.localization_token].view(1, 1, d).expand(B, 1, d)
        add = torch.cat([pose_emb, lpe], 1)                                             # [B,S+1,d]
        mask = torch.full_like(codes[:, :1], self.mask_token)
        ids = torch.cat([codes[:, :-1], mask, codes[:, -1:]], 1)                        # [B,S+1,t,t]
        if self.prune_last_block:
            hf = self._blocks(ids, add, B, S + 1, L, mask_spec=S - 1, tail_views=2).view(B, 2, L, d)      # the MASK view and the LOC view
            h_mask = hf[:, 0].contiguous().view(B * L, d)
            h_loc = hf[:, 1].contiguous().view(B * L, d)
        else:
            hf = self._blocks(ids, add, B, S + 1, L, mask_spec=S - 1).view(B, S + 1, L, d)
            h_mask = hf[:, S - 1].contiguous().view(B * L, d)
            h_loc = hf[:, S].contiguous().view(B * L, d)
        gen = self._lm_argmax(h_mask, B * L) if codes_only else None
        if gen is None:
            lg = torch.empty((B * L, nE), dtype=torch.float32, device=dev)
            self._lm(h_mask, B * L, lg)                                                 # migt.py:417
            gen = ops.argmax_rows(lg, B * L, nE) if codes_only else None
        p1 = self._gemm(h_loc, 'pose_criterion.pose_classifier.c_fc', B * L, epilogue=ops.EPI_GELU)
        p2 = self._gemm(p1, 'pose_criterion.pose_classifier.c_proj', B * L)
        pose = geometry.pose_head_postprocess(p2.view(B, 1, L, 7), c.pose_multiplier)
        return (gen.view(B, *tshape) if codes_only else lg.view(B, *tshape, nE)), pose

    def _call_streams(self, ids, pose_emb, loc_tokens, out_poses, B, S, L, orig_shape):
        """Multi-stream ("branching") forward, migt.py:371-455 with training=False.

        Streams are laid out as extra views of one sequence (view index = stream*S + position) and the attention
        kernel's STREAMS mask gives a branch position i the main views < i plus its own tile — i.e.
        compute_causal_block_multiend_attention for every stream in one launch per layer.  Weights are shared
        across streams exactly as in Block.call (migt.py:230-238)."""
        c, dev = self.config, self.device
        d, nE = c.d_model, c.n_embeddings
        ids_streams = [ids.reshape(B, S, L)]
        add_streams = [pose_emb]
        img_ptr = pose_ptr = 0
        if out_poses is not None:                                            # migt.py:382-385,393-396
            out_poses = out_poses.to(dev)
            if out_poses.shape[1] != S:
                raise ValueError('output_poses must have one pose per view')
            ids_streams.append(torch.full((B, S, L), self.mask_token, dtype=ids.dtype, device=dev))
            add_streams.append(self._pose_embed(out_poses))
            img_ptr = len(ids_streams) - 1
        if loc_tokens is not None:                                           # migt.py:378-381,398-401
            lt = loc_tokens.to(dev).reshape(B, -1, L)
            if lt.shape[1] != S:
                raise ValueError('localization_tokens must have one token map per view')
            ids_streams.append(lt.to(ids.dtype))
            add_streams.append(self._wte[self.localization_token].view(1, 1, d).expand(B, S, d))
            pose_ptr = len(ids_streams) - 1
        NS = len(ids_streams)
        if NS > 1 and S == 1:
            # one view per stream: a branch position 0 sees no main view (j < 0) and its own tile, the main view sees itself — every
            # (scene, stream) is an independent 1-view sequence.  The kernels' STREAMS encoding (-S <= -2) cannot say S = 1 (-1 is
            # plain block-causal, where the streams would see each other), so run them as B*NS scenes of one view: same rows exactly.
            hf = self._blocks(torch.cat(ids_streams, 1), torch.cat(add_streams, 1), B * NS, 1, L, mask_spec=-1).view(B, NS, S, L, d)
        else:
            hf = self._blocks(torch.cat(ids_streams, 1), torch.cat(add_streams, 1), B, NS * S, L,
                              mask_spec=(-S if NS > 1 else -1)).view(B, NS, S, L, d)
        out = dict(hidden_states=[hf[:, s] for s in range(NS)])
        M = B * S * L
        hi = hf[:, img_ptr].contiguous().view(M, d)
        lg = torch.empty((M, nE), dtype=torch.float32, device=dev)
        self._lm(hi, M, lg)                                                  # migt.py:417
        out['logits'] = lg.view(*orig_shape, nE)
        if self.use_localization:                                            # migt.py:430-451
            hp = hf[:, pose_ptr].contiguous().view(M, d)
            p1 = self._gemm(hp, 'pose_criterion.pose_classifier.c_fc', M, epilogue=ops.EPI_GELU)
            p2 = self._gemm(p1, 'pose_criterion.pose_classifier.c_proj', M)
            out['pose_prediction'] = geometry.pose_head_postprocess(p2.view(B, S, L, 7), c.pose_multiplier)
        out['loss'] = 0
        return out

    # ------------------------------------------------------------------ forward (single stream, inference)
    def __call__(self, inputs, training=False, compute_losses=False, last_view_logits_only=False, last_view_codes_only=False):
        if training:
            raise RuntimeError('the training graph (dropout, losses, backward, optimizer: MIGT.train_step migt.py:464-505) is '
                               'viewformer_amd.train.MIGTTrainer(model).train_step(poses, tokens); __call__ is inference')
        if self._sd_host is None or self.device is None:
            raise RuntimeError('MIGT: load_state_dict() and .to("cuda") first')
        c, dev = self.config, self.device
        ids = inputs['input_ids'].to(dev)
        poses = inputs['poses'].to(dev)
        if poses.dtype != torch.float32:
            raise TypeError('poses must be float32 (migt.py:346)')
        orig_shape = tuple(ids.shape)
        B, S = orig_shape[:2]
        L = int(np.prod(orig_shape[2:]))
        d, H = c.d_model, c.n_head
        M = B * S * L
        if d // H != 64:
            raise ops._lib.VfError('attention kernel supports head dim 64 only')

        pose_emb = self._pose_embed(poses)                                   # [B,Sp,d]
        Sp = pose_emb.shape[1]
        if self.use_localization and S - Sp > 0:                             # migt.py:387-390
            lpe = self._wte[self.localization_token].view(1, 1, d).expand(B, S - Sp, d)
            pose_emb = torch.cat([pose_emb, lpe], 1)
        elif Sp != S:
            raise ValueError(f'poses has {Sp} views but input_ids has {S}')

        # ---- optional branch streams (migt.py:371-401): MASK stream for images, LOC stream for poses ----------
        loc_tokens = inputs.get('localization_tokens')
        out_poses = inputs.get('output_poses')
        if compute_losses:                                                   # forward graph of the training step
            if loc_tokens is None and self.use_localization:
                loc_tokens = ids
            if out_poses is None:
                out_poses = poses
        if loc_tokens is not None or out_poses is not None:
            if last_view_logits_only or last_view_codes_only:
                raise ValueError('last_view_logits_only / last_view_codes_only apply to the single-stream call')
            return self._call_streams(ids, pose_emb, loc_tokens, out_poses, B, S, L, orig_shape)

        hf = self._blocks(ids, pose_emb, B, S, L)

        out = dict(hidden_states=[hf.view(B, S, L, d)])
        nE = c.n_embeddings
        if last_view_codes_only:
            last_view_logits_only = True
        if last_view_logits_only:
            hl = hf.view(B, S, L, d)[:, -1].contiguous().view(B * L, d)
            gen = self._lm_argmax(hl, B * L) if last_view_codes_only else None
            if gen is None:
                lg = torch.empty((B * L, nE), dtype=torch.float32, device=dev)
                self._lm(hl, B * L, lg)
                out['logits_last'] = lg.view(B, *orig_shape[2:], nE)
                if last_view_codes_only:
                    gen = ops.argmax_rows(lg, B * L, nE)
            if gen is not None:
                out['codes_last'] = gen.view(B, *orig_shape[2:])                  # argmax(logits, -1)[:, -1], evaluate_transformer.py:123
        else:
            lg = torch.empty((M, nE), dtype=torch.float32, device=dev)
            self._lm(hf, M, lg)                                              # migt.py:417,51-56
            out['logits'] = lg.view(*orig_shape, nE)
        if self.use_localization:                                            # migt.py:430-451
            if last_view_logits_only:      # pose head on the last view only: shape [B,1,L,7], so [:, -1:] still works
                hp, Mp, Sp_out = hf.view(B, S, L, d)[:, -1].contiguous().view(B * L, d), B * L, 1
            else:
                hp, Mp, Sp_out = hf, M, S
            p1 = self._gemm(hp, 'pose_criterion.pose_classifier.c_fc', Mp, epilogue=ops.EPI_GELU)
            p2 = self._gemm(p1, 'pose_criterion.pose_classifier.c_proj', Mp)
            out['pose_prediction'] = geometry.pose_head_postprocess(p2.view(B, Sp_out, L, 7), c.pose_multiplier)
        out['loss'] = 0
        return out
