"""CPU: the 7-Scenes localization evaluator's host side (viewformer_amd/evaluate_sevenscenes.py) against restatements of
viewformer/evaluate/evaluate_sevenscenes.py written here and in tests/sevenscenes_ref.py, and the C-ABI of the camera k-NN kernel
without a GPU (argument validation happens before any launch; pointers are never dereferenced)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import sevenscenes_ref as ref


# ------------------------------------------------------------------------------------------------ pose distance
def test_camera_distances_room_family_within_measured_tolerance():
    """all N rows of 16 queries within tol = 4 x the literal fp32 formula's largest error (top-(k + 1) = every row here).
    Measured: tol 3.8e-6, largest error of compute_camera_distances 9.4e-7."""
    from viewformer_amd.evaluate_sevenscenes import compute_camera_distances
    db, q = ref.cameras('room', 1000, 0), ref.cameras('room', 16, 1)
    d64 = ref.distances64(db, q)
    tol = ref.tolerance(db, q, k=db.shape[0], d64=d64)
    got = compute_camera_distances(torch.from_numpy(db), torch.from_numpy(q)[:, None])
    assert got.dtype == torch.float32 and tuple(got.shape) == (16, 1000)
    err = float(np.abs(got.numpy().astype(np.float64) - d64).max())
    print(f'room: tol {tol:.2e}, max error {err:.2e}')
    assert 0 < tol < 1e-5                      # the yardstick itself is an fp32-level number
    assert err <= tol
    # the reference's own shape: one [1,7] camera against the database
    one = compute_camera_distances(torch.from_numpy(db), torch.from_numpy(q[:1]))
    assert torch.equal(one, got[0])


def test_camera_distances_free_family_finite_and_within_the_literals_error_class():
    """free orientations reach relative rotations near pi, where asin is ill-conditioned: finite everywhere (the clamp), and within
    4 x the literal's own largest error on these inputs.  Measured: literal 8.9e-4 (bound 3.6e-3), compute_camera_distances 8.9e-4."""
    from viewformer_amd.evaluate_sevenscenes import compute_camera_distances
    db, q = ref.cameras('free', 1000, 2), ref.cameras('free', 16, 3)
    d64 = ref.distances64(db, q)
    lit = ref.distances32_literal(db, q).astype(np.float64)
    lit_err = float(np.nanmax(np.abs(lit - d64)))                 # (the literal may be NaN where the norm rounds above 1)
    got = compute_camera_distances(torch.from_numpy(db), torch.from_numpy(q)[:, None]).numpy().astype(np.float64)
    err = float(np.abs(got - d64).max())
    print(f'free: literal max error {lit_err:.2e}, compute_camera_distances max error {err:.2e}')
    assert np.isfinite(got).all()
    assert err <= 4 * lit_err
    # a query identical to a database row: distance ~ 0, and an exactly antipodal orientation: the clamp's case
    same = compute_camera_distances(torch.from_numpy(db), torch.from_numpy(db[7:8]))
    assert int(same.argmin()) == 7 and float(same[7]) < 1e-3
    a = torch.tensor([[0., 0., 0., 1., 0., 0., 0.]])
    b = torch.tensor([[0., 0., 0., 0., 0.6, 0.8, 0.]])
    b[0, 3:] = b[0, 3:] * 1.0000001
    r = float(compute_camera_distances(a, b))
    assert np.isfinite(r) and abs(r - np.pi) < 2e-3            # (asin's slope is unbounded at 1: a ulp of the norm is ~5e-4 of the angle)


# ------------------------------------------------------------------------------------------------ generate_other_viewpoints
def _relative_angle(q_new, q_old):
    dot = np.abs((q_new * q_old).sum(-1) / (np.linalg.norm(q_new, axis=-1) * np.linalg.norm(q_old, axis=-1)))
    return 2 * np.arccos(np.minimum(dot, 1.0))


def test_generate_other_viewpoints_matches_the_literal_restatement():
    from viewformer_amd.evaluate_sevenscenes import generate_other_viewpoints, default_uniforms
    g = np.random.default_rng(4)
    for shape in ((1, 1), (5, 1), (3, 2)):
        cam = ref.cameras('free', int(np.prod(shape)), 5).reshape(*shape, 7)
        u = g.random(size=(*shape, 8)).astype(np.float32)
        got = generate_other_viewpoints(torch.from_numpy(cam), torch.from_numpy(u))
        want = ref.other_viewpoints_literal(cam, u)
        assert got.dtype == torch.float32 and tuple(got.shape) == (*shape, 7)
        assert np.abs(got.numpy() - want).max() < 2e-6
        assert (_relative_angle(got.numpy()[..., 3:].astype(np.float64), cam[..., 3:].astype(np.float64)) <= 0.3 + 1e-3).all()
        assert (np.linalg.norm(got.numpy()[..., :3] - cam[..., :3], axis=-1) <= 1.0 + 1e-5).all()
    # 5 cameras: whole-tensor normalisation (sic) is not per-row normalisation
    cam = ref.cameras('room', 5, 6).reshape(5, 1, 7)
    u = g.random(size=(5, 1, 8)).astype(np.float32)
    got = generate_other_viewpoints(torch.from_numpy(cam), torch.from_numpy(u)).numpy()
    offs = np.linalg.norm(got[..., :3] - cam[..., :3], axis=-1)
    d = u[..., 0:3].astype(np.float64) * 2 - 1
    whole = np.linalg.norm(d, axis=-1) / np.sqrt((d * d).sum()) * u[..., 6]          # what :25,:28 give
    per_row = u[..., 6].astype(np.float64)                                          # what a per-camera normalisation would give
    assert np.abs(offs - whole).max() < 1e-5
    assert np.abs(offs - per_row).max() > 0.05
    # one camera: the offset has exactly the drawn length and the rotation the drawn angle
    one = generate_other_viewpoints(torch.from_numpy(cam[:1]), torch.from_numpy(u[:1])).numpy()
    assert abs(np.linalg.norm(one[0, 0, :3] - cam[0, 0, :3]) - u[0, 0, 6]) < 1e-5
    assert abs(_relative_angle(one[..., 3:].astype(np.float64), cam[:1, :, 3:].astype(np.float64))[0, 0] - 0.3 * u[0, 0, 7]) < 1e-3
    # default draws: the counter hash — reproducible, seed-dependent, in [0, 1)
    u0 = default_uniforms((5, 1), seed=7)
    assert tuple(u0.shape) == (5, 1, 8) and float(u0.min()) >= 0 and float(u0.max()) < 1
    assert torch.equal(u0, default_uniforms((5, 1), seed=7)) and not torch.equal(u0, default_uniforms((5, 1), seed=8))
    a = generate_other_viewpoints(torch.from_numpy(cam), seed=7)
    assert torch.equal(a, generate_other_viewpoints(torch.from_numpy(cam), u0))
    with pytest.raises(ValueError):
        generate_other_viewpoints(torch.from_numpy(cam), u0[:4])


# ------------------------------------------------------------------------------------------------ batches from a bank
class FakeBank:
    """a bank's host side: arrays only"""

    def __init__(self, n, keep_frames=True, seed=0):
        g = np.random.default_rng(seed)
        self.files = [f'seq-01/frame-{i:06d}.color.png' for i in range(n)]
        self._lookup = {x: i for i, x in enumerate(self.files)}
        self.cameras_host = ref.cameras('room', n, seed)
        self.frames = torch.from_numpy(g.integers(0, 256, size=(n, 4, 4, 3), dtype=np.uint8)) if keep_frames else None

    def index(self, name):
        return self._lookup[name]

    def __len__(self):
        return len(self.files)


def test_build_batch_order_matches_and_fill(tmp_path):
    from viewformer_amd.evaluate_sevenscenes import build_batch, load_image_match_map, draw_fill_indices
    bank = FakeBank(40)
    gt_frames = torch.full((1, 4, 4, 3), 7, dtype=torch.uint8)
    gt_cameras = ref.cameras('room', 1, 9)
    # match map file: '<query> <match>' lines, matches kept in file order
    p = tmp_path / 'matches.txt'
    p.write_text(''.join(f'q/frame-000001.color.png {bank.files[i]}\n' for i in (30, 3, 17, 5)) + f'q/frame-000002.color.png {bank.files[9]}\r\n')
    mm = load_image_match_map(str(p))
    assert mm['q/frame-000001.color.png'] == [bank.files[i] for i in (30, 3, 17, 5)] and mm['q/frame-000002.color.png'] == [bank.files[9]]
    # the reference's build_batch (:234-244), restated: matches[:top_n] ++ random.sample(files, 19 - len)
    rng = random.Random(3)
    want = mm['q/frame-000001.color.png'][:3]
    want = want + rng.sample(bank.files, 19 - len(want))
    want_idx = [bank.files.index(x) for x in want]
    cameras, frames, indices = build_batch(bank, gt_frames, gt_cameras, mm['q/frame-000001.color.png'], rng=random.Random(3), top_n=3)
    assert indices == want_idx and indices[:3] == [30, 3, 17]
    assert tuple(cameras.shape) == (1, 20, 7) and cameras.dtype == torch.float32
    assert np.array_equal(cameras[0, :19].numpy(), bank.cameras_host[want_idx]) and np.array_equal(cameras[0, 19].numpy(), gt_cameras[0])
    assert tuple(frames.shape) == (1, 20, 4, 4, 3)
    assert torch.equal(frames[0, :19], bank.frames[want_idx]) and torch.equal(frames[0, 19], gt_frames[0])     # context first, query last
    # no matches, a short context, a bank without pixels: the query frame alone comes back
    cameras, frames, indices = build_batch(FakeBank(40, keep_frames=False), gt_frames, gt_cameras, context_size=4, rng=random.Random(5))
    assert indices == [bank.files.index(x) for x in random.Random(5).sample(bank.files, 4)]
    assert tuple(cameras.shape) == (1, 5, 7) and tuple(frames.shape) == (1, 1, 4, 4, 3) and len(set(indices)) == 4
    assert tuple(build_batch(bank, gt_frames, gt_cameras, context_size=4, rng=random.Random(5), context_frames=False)[1].shape) == (1, 1, 4, 4, 3)
    # the refinement's fill (:191): a sample WITHOUT replacement over the bank's files, drawn from the caller's generator
    assert draw_fill_indices(bank, 10, random.Random(11)) == [bank.files.index(x) for x in random.Random(11).sample(bank.files, 10)]
    with pytest.raises(ValueError):
        draw_fill_indices(bank, 41, random.Random(0))


# ------------------------------------------------------------------------------------------------ C-ABI without a GPU
@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()
    return _lib.load()


def test_camera_knn_abi_validation_without_gpu(lib):
    d = ctypes.c_void_p(4096)              # never dereferenced
    knn, ws = lib.vf_camera_knn_f32, lib.vf_camera_knn_workspace_bytes
    assert lib.vf_abi_version() == 20      # the addition is additive
    assert knn(d, 7000, d, 4, 0, 0.3, d, d, d, None) == -1             # k = 0
    assert knn(d, 7000, d, 4, 33, 0.3, d, d, d, None) == -2            # k = 33: unsupported
    assert knn(d, 8, d, 4, 9, 0.3, d, d, d, None) == -1                # N < k
    assert knn(d, 7000, d, -1, 9, 0.3, d, d, d, None) == -1            # Q < 0
    assert knn(d, 1 << 31, d, 4, 9, 0.3, d, d, d, None) == -2          # N > 2^31 - 1
    assert knn(None, 7000, d, 4, 9, 0.3, d, d, d, None) == -1          # NULL db
    assert knn(d, 7000, None, 4, 9, 0.3, d, d, d, None) == -1          # NULL queries
    assert knn(d, 7000, d, 4, 9, 0.3, None, d, d, None) == -1          # NULL idx
    assert knn(d, 7000, d, 4, 9, 0.3, d, d, None, None) == -1          # NULL workspace where one is needed
    assert knn(d, 7000, d, 4, 9, 0.3, d, d, ctypes.c_void_p(4100), None) == -1     # workspace alignment
    assert knn(d, 7000, d, 4, 9, -0.5, d, d, d, None) == -1            # negative weight: keys would not order
    assert knn(d, 7000, d, 4, 9, float('nan'), d, d, d, None) == -1
    assert knn(d, 7000, d, 0, 9, 0.3, d, None, d, None) == 0           # Q = 0: a no-op
    assert knn(None, 7000, None, 0, 9, 0.3, None, None, None, None) == 0
    # workspace: [Q][tiles of 1024 rows][k] 8-byte keys; none for a single tile; monotone in N; 0 for invalid shapes
    assert ws(7000, 64, 9) == 64 * 7 * 9 * 8 and ws(1024, 64, 9) == 0 and ws(1025, 1, 1) == 2 * 8
    sizes = [ws(n, 16, 19) for n in (19, 1000, 1024, 1025, 7000, 100000, 250001, (1 << 31) - 1)]
    assert sizes == sorted(sizes) and sizes[-1] == 16 * (1 << 21) * 19 * 8
    assert ws(7000, 4, 0) == 0 and ws(7000, 4, 33) == 0 and ws(8, 4, 9) == 0 and ws(7000, -1, 9) == 0 and ws(1 << 31, 4, 9) == 0
    assert ws(7000, 0, 9) == 0


def test_camera_knn_refuses_cpu_tensors(lib):
    from viewformer_amd import ops, _lib
    with pytest.raises(_lib.VfError):
        ops.camera_knn(torch.zeros(10, 7), torch.zeros(1, 7), 3)
    with pytest.raises(ValueError):
        ops.camera_knn(torch.zeros(10, 6), torch.zeros(1, 7), 3)
