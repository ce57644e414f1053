"""Test infrastructure of the 7-Scenes evaluator's tests (CPU and GPU): seeded camera families, the fp64 numpy transliteration of the
reference's pose distance (viewformer/evaluate/evaluate_sevenscenes.py:36-45), the literal fp32 formula on plain torch-CPU ops, the
tolerance the tests derive from the two, and the literal numpy restatement of ``generate_other_viewpoints`` (:20-33)."""
import numpy as np
import torch

POS_WEIGHT = 0.3


def cameras(family, n, seed):
    """[n,7] float32, positions ~ N(0, 1.5).  'free': random unit quaternions with w >= 0.  'room': rotations by an angle in [0, 1.2] rad
    about a random axis from the identity (a hand-held camera in a room): the relative rotation of two such cameras stays below 2.4 rad,
    the asin argument below sin(1.2) = 0.94, away from asin's ill-conditioned end."""
    g = np.random.default_rng(seed)
    pos = g.normal(0.0, 1.5, size=(n, 3))
    if family == 'free':
        q = g.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        q *= np.where(q[:, :1] >= 0, 1.0, -1.0)
    elif family == 'room':
        axis = g.normal(size=(n, 3))
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        angle = g.uniform(0.0, 1.2, size=(n, 1))
        q = np.concatenate((np.cos(angle / 2), np.sin(angle / 2) * axis), -1)
    else:
        raise ValueError(family)
    return np.concatenate((pos, q), -1).astype(np.float32)


def _hamilton(q1, q2, stack):
    """geometry_tf.py:6-13, term for term and in its order"""
    w1, x1, y1, z1 = (q1[..., i] for i in range(4))
    w2, x2, y2, z2 = (q2[..., i] for i in range(4))
    x = x1 * w2 + y1 * z2 - z1 * y2 + w1 * x2
    y = -x1 * z2 + y1 * w2 + z1 * x2 + w1 * y2
    z = x1 * y2 - y1 * x2 + z1 * w2 + w1 * z2
    w = -x1 * x2 - y1 * y2 - z1 * z2 + w1 * w2
    return stack((w, x, y, z), -1)


def distances64(db, queries, pos_weight=POS_WEIGHT):
    """:36-45 in float64 numpy: db [N,7], queries [Q,7] -> [Q,N].  (The norm of a unit quaternion's vector part can round a ulp above 1 in
    any precision; it is clamped as the feature clamps it, so that the yardstick has no NaN of its own.)"""
    db = np.asarray(db, np.float64)[None]
    q = np.asarray(queries, np.float64)[:, None]
    pos = np.linalg.norm(db[..., :3] - q[..., :3], axis=-1)

    def l2n(x):
        return x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12))
    x1, x2 = np.broadcast_arrays(l2n(db[..., 3:]), l2n(q[..., 3:]))
    conj = np.concatenate((x2[..., :1], -x2[..., 1:]), -1)
    diff = _hamilton(x1, conj, np.stack)
    quat = 2 * np.arcsin(np.minimum(np.linalg.norm(diff[..., 1:], axis=-1), 1.0))
    return pos * pos_weight + quat


def distances32_literal(db, queries, pos_weight=POS_WEIGHT):
    """the literal fp32 formula on plain torch-CPU ops in the reference's operation order (no clamp: NaN where the norm rounds above 1)"""
    db = torch.as_tensor(np.asarray(db, np.float32))[None]
    q = torch.as_tensor(np.asarray(queries, np.float32))[:, None]
    d = db[..., :3] - q[..., :3]
    pos = torch.sqrt((d * d).sum(-1))

    def l2n(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12))
    x1, x2 = torch.broadcast_tensors(l2n(db[..., 3:]), l2n(q[..., 3:]))
    conj = torch.cat((x2[..., :1], -x2[..., 1:]), -1)
    v = _hamilton(x1, conj, torch.stack)[..., 1:]
    quat = 2 * torch.asin(torch.sqrt((v * v).sum(-1)))
    return (pos * pos_weight + quat).numpy()


def top_rows(d64, k):
    """per query the indices of its k smallest fp64 distances, stable (ties to the lowest index): [Q,k]"""
    return np.argsort(d64, axis=-1, kind='stable')[:, :k]


def tolerance(db, queries, k, d64=None):
    """4 x the largest |literal fp32 - fp64| over every query's fp64 top-(k + 1) rows (all rows when k + 1 >= N).  The factor 4 covers
    another association of the Hamilton product's sums and a device's asin / sqrt against libm's."""
    d64 = distances64(db, queries) if d64 is None else d64
    lit = distances32_literal(db, queries).astype(np.float64)
    rows = top_rows(d64, min(k + 1, d64.shape[1]))
    err = np.abs(np.take_along_axis(lit, rows, -1) - np.take_along_axis(d64, rows, -1))
    assert np.isfinite(err).all(), 'the literal formula is not finite on a row that ranks first'
    return 4.0 * float(err.max())


def other_viewpoints_literal(camera, uniforms):
    """:20-33 in float64 numpy with the draws given: camera [...,7], uniforms [...,8] in [0,1).  tf.math.l2_normalize without an axis
    normalises over the WHOLE tensor (sic)."""
    camera, u = np.asarray(camera, np.float64), np.asarray(uniforms, np.float64)

    def l2n_all(x):
        return x / np.sqrt(max(float((x * x).sum()), 1e-12))
    pos_offset = l2n_all(u[..., 0:3] * 2 - 1)
    axis = l2n_all(u[..., 3:6] * 2 - 1)
    pos_offset = pos_offset * (u[..., 6:7] * 1.0)
    angle = u[..., 7:8] * 0.3
    rot = np.concatenate((np.cos(angle / 2), np.sin(angle / 2) * axis), -1)
    q = _hamilton(rot, camera[..., 3:], np.stack)
    q = q / np.sqrt(np.maximum((q * q).sum(-1, keepdims=True), 1e-12))
    return np.concatenate((pos_offset + camera[..., :3], q), -1)
