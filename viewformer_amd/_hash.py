"""Host-side evaluation of the counter hashes of csrc/vf_common.h: ``vf_dropout_hash`` for the few per-scene random numbers the
training step draws on the host (random pose multiplier), and the dropout-mask definition itself (``vf_dropout_word`` /
``vf_dropout_keep``) for host-side checks; the masks of a training step are evaluated inside the kernels.

Mask definition (round 4): elements come in GROUPS of four that share one 32-bit word,
    word(seed, site, g) = lowbias32(lo32(g) ^ vf_dropout_hash(seed, site, hi32(g)))        g = 64-bit group index
    keep(element j of group g) = rotl32(word, 8 j) >= floor(rate * 2^32)
so every element's keep probability is exactly 1 - floor(rate 2^32) / 2^32 (a rotation of a uniform word is uniform) and a lane that
holds the four elements of a group pays for one hash.  Group index and position of an element:
    [M][N] activations (embedding / residual / MLP sites):  g = (m >> 2) * N + n,  j = m & 3    (four consecutive ROWS of a column:
        what a lane of the GEMM epilogue holds);
    attention weights (b, h, q, k) of a T-token sequence:  g = ((b H + h) << 32) | (q * ceil(T / 4) + (k >> 2)),  j = k & 3.

Sampling noise (csrc/sample_rows.hip: vf_sample_rows_f32), built from the same two hashes: code n of the row with 64-bit ``row_id``, sample
s (0 <= s < 65536) gets
    key = vf_dropout_hash(seed, SITE_SAMPLE + s, row_id)        SITE_SAMPLE = 0x5A0000
    w_n = lowbias32(n ^ key)
    u_n = ((w_n >> 9) + 0.5) * 2^-23                            strictly inside (0, 1), exact in fp32 (and 1 - u_n is, too)
    g_n = -log(-log u_n)                                        standard Gumbel noise
and the draw is the arg-max over the kept codes of logit / temperature + g (Gumbel-max: an exact draw from their soft-max).  A token's
noise depends on (seed, row_id, s, n) and on nothing else: not on the launch's geometry, the number of samples or the chunking."""
import numpy as np

_M = 0xFFFFFFFF
SITE_SAMPLE = 0x5A0000


def dropout_hash(seed, site, idx):
    """uint32 hash of (seed, site, 64-bit element index); ``idx`` array-like -> uint32 array"""
    out = []
    for i in np.asarray(idx, dtype=np.uint64).reshape(-1).tolist():
        h = (int(seed) ^ ((int(site) * 0x9E3779B9) & _M)) & _M
        h ^= i & _M
        h = (h * 0x85EBCA6B) & _M
        h ^= h >> 13
        h = (h + (((i >> 32) * 0xC2B2AE35) & _M) + 0x27D4EB2F) & _M
        h ^= h >> 16
        h = (h * 0x165667B1) & _M
        h ^= h >> 15
        h = (h * 0xD3A2646C) & _M
        h ^= h >> 16
        out.append(h)
    return np.asarray(out, dtype=np.uint32)


def lowbias32(x):
    """Chris Wellons' 2-multiply integer hash (bias 0.17): uint32 array -> uint32 array"""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(_M)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(_M)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(_M)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def dropout_word(seed, site, group):
    """the 32-bit word shared by the four elements of 64-bit group index ``group`` (array-like)"""
    g = np.asarray(group, dtype=np.uint64)
    hi = (g >> np.uint64(32)).reshape(-1)
    keys = {int(h): int(dropout_hash(seed, site, [h])[0]) for h in np.unique(hi).tolist()}
    key = np.asarray([keys[int(h)] for h in hi.tolist()], dtype=np.uint64).reshape(g.shape)
    return lowbias32((g & np.uint64(_M)) ^ key)


def dropout_keep(seed, site, group, sub, rate):
    """bool keep mask: rotl32(word(group), 8 * sub) >= floor(rate * 2^32)"""
    w = dropout_word(seed, site, group).astype(np.uint64)
    sh = (np.asarray(sub, dtype=np.uint64) & np.uint64(3)) * np.uint64(8)
    rot = ((w << sh) | (w >> (np.uint64(32) - sh))) & np.uint64(_M)
    rot = np.where(sh == 0, w, rot)
    return rot >= np.uint64(int(rate * 4294967296.0))


def elem_group(m, n, N):
    """(group, sub) of element (m, n) of an [M][N] activation"""
    m = np.asarray(m, dtype=np.uint64)
    g = (m >> np.uint64(2)) * np.uint64(N) + np.asarray(n, dtype=np.uint64)
    return g, np.broadcast_to(m & np.uint64(3), g.shape)


def attn_group(plane, q, k, T):
    """(group, sub) of attention weight (plane = b H + h, q, k) of a T-token sequence"""
    k = np.asarray(k, dtype=np.uint64)
    stride = np.uint64((T + 3) // 4)
    g = (np.asarray(plane, dtype=np.uint64) << np.uint64(32)) | (np.asarray(q, dtype=np.uint64) * stride + (k >> np.uint64(2)))
    return g, np.broadcast_to(k & np.uint64(3), g.shape)


def sample_key(seed, row_id, s):
    """the 32-bit key of sample ``s`` of the row with 64-bit ``row_id``"""
    if not 0 <= int(s) < 65536:
        raise ValueError(f'sample_key: 0 <= s < 65536 expected, got {s}')
    return int(dropout_hash(seed, SITE_SAMPLE + int(s), [int(row_id) & 0xFFFFFFFFFFFFFFFF])[0])


def sample_uniform(seed, row_id, s, N):
    """u_n for n < N, float64 holding the exact fp32 values ((w_n >> 9) + 0.5) * 2^-23"""
    w = lowbias32(np.arange(N, dtype=np.uint64) ^ np.uint64(sample_key(seed, row_id, s)))
    return ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def sample_gumbel(seed, row_id, s, N):
    """g_n = -log(-log u_n) in float64 from the exact u (-log u through log1p of the exact 1 - u: accurate where u is close to 1)"""
    u = sample_uniform(seed, row_id, s, N)
    return -np.log(-np.log1p(-(1.0 - u)))
