"""Shared by tests/test_context_lengths_host.py and tests/test_hip_context_lengths.py: the fp64 prefix attention with a context length per
query view, and the kernel cases.  No device is needed to import or to run this."""
import numpy as np
import torch

L = 64


def rand(shape, seed, scale):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def attn_fp64_lengths(qkv_ctx, qkv_q, B, H, C, N, lengths, L=L):
    """``_attn_fp64`` of tests/test_hip_render.py with a length per view: query view (b, n) against the first lengths[b][n] * L context
    keys of its scene and the L keys of its own view, fp64; thirds (V, Q, K).  The keys of views >= its length are REMOVED from the
    softmax, not masked with a large negative.  ``lengths`` [B,N] (anything ``np.asarray`` takes).  -> [B*N*L, H*64] float64"""
    d = H * 64
    lengths = np.asarray(lengths).reshape(B, N)
    ctx = qkv_ctx.double().cpu().view(B, C * L, 3, H, 64)
    qq = qkv_q.double().cpu().view(B, N, L, 3, H, 64)
    out = torch.empty((B, N, L, H, 64), dtype=torch.float64)
    for b in range(B):
        for n in range(N):
            c = int(lengths[b, n])
            assert 0 <= c <= C
            q, k, v = (qq[b, n, :, i].permute(1, 0, 2) for i in (1, 2, 0))                       # [H,L,64]
            kk = torch.cat([ctx[b, :c * L, 2].permute(1, 0, 2), k], 1)                           # [H,c*L+L,64]
            vv = torch.cat([ctx[b, :c * L, 0].permute(1, 0, 2), v], 1)
            p = torch.softmax(q @ kk.transpose(-1, -2), -1)                                      # un-scaled scores
            out[b, n] = (p @ vv).permute(1, 0, 2)
    return out.reshape(B * N * L, d)


def _random_lengths():
    """(2,2,6,9): seeded random in 0...6, the second group of four views of scene 0 (views 4...7: a whole group of the bf16 arm, two whole
    groups of the f32eq arm) forced to one length"""
    g = np.random.Generator(np.random.PCG64(606))
    a = g.integers(0, 7, size=(2, 9))
    a[0, 4:8] = 4
    return a.tolist()


# ((B, H, C, N), lengths [B][N]): the smallest shapes that reach every branch of the kernels
KERNEL_CASES = [
    ((1, 2, 3, 5), [[0, 3, 1, 3, 2]]),                          # a mixed group plus a one-view tail group
    ((2, 3, 1, 1), [[0], [1]]),                                 # lengths per scene
    ((1, 2, 2, 4), [[0, 0, 0, 0]]),                             # groups with no prefix step: the first prefetch fetches an own tile
    ((2, 2, 6, 9), _random_lengths()),
    ((1, 12, 19, 8), [[0, 19, 1, 18, 5, 5, 12, 7]]),
]
KERNEL_ARMS = ['bf16', 'bf16-f32io', 'f32eq']


def case_id(case):
    (B, H, C, N), _ = case
    return f'B{B}-H{H}-C{C}-N{N}'
