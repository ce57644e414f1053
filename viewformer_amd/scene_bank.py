"""Scene bank of the 7-Scenes localization evaluator: one scene's training views, encoded ONCE and kept on the GPU.

The reference's ``SceneLookup`` (viewformer/evaluate/evaluate_sevenscenes.py:48-68) keeps the training cameras, file names and image
loaders of a scene on the host; every query then stacks 19 context frames, uploads them and runs them through the encoder again
(:192-197, :240-244).  Codes are a pure function of the frame (the encoder is batch-invariant), so the bank encodes the scene's frames
once, in chunks, and keeps ``codes`` int32 [N,t,t] and ``cameras`` fp32 [N,7] on the device: a query's context is a gather, and the
pose refinement's search over every training camera (``compute_camera_distances`` + ``tf.argsort``, :188-189) is one kernel
(``ops.camera_knn``) on the stream.  File names and the name -> index map of ``SceneLookup.__getitem__`` stay on the host.  Reading
7-Scenes files from disk is the caller's business: the bank takes arrays.
"""
import numpy as np
import torch

from . import ops
from .evaluate import _frames_for_encode

POS_WEIGHT = 0.3               # "Coefficient chosen arbitrary", evaluate_sevenscenes.py:44-45


class SceneBank:
    """``frames_u8`` [N,H,W,3] uint8 (host or device; resized for the encoder as the evaluators do, the reference loads the scene at
    128), ``cameras`` [N,7] (xyz + quaternion w,x,y,z), ``files``: N names (default ``frame-%06d.color.png``).  ``batch_size`` frames
    are encoded per call.  ``keep_frames``: keep a REFERENCE to ``frames_u8`` where the caller had it (no copy) for the evaluators that
    need pixels (``frames_at``: the re-encoding arm of the refinement, the multi-context loop)."""

    def __init__(self, codebook_model, frames_u8, cameras, files=None, batch_size: int = 64, keep_frames: bool = True):
        dev = codebook_model.device
        frames_u8 = torch.as_tensor(frames_u8)
        cameras_host = np.ascontiguousarray(np.asarray(torch.as_tensor(cameras).cpu(), dtype=np.float32))
        N = frames_u8.shape[0]
        if frames_u8.dim() != 4 or frames_u8.dtype != torch.uint8 or cameras_host.shape != (N, 7) or N == 0 or batch_size < 1:
            raise ValueError(f'SceneBank: frames uint8 [N,H,W,3] and cameras [N,7] expected, got {tuple(frames_u8.shape)} '
                             f'{frames_u8.dtype} and {cameras_host.shape}')
        self.files = [f'frame-{i:06d}.color.png' for i in range(N)] if files is None else list(files)
        if len(self.files) != N:
            raise ValueError(f'SceneBank: {len(self.files)} file names for {N} frames')
        self._lookup = {x: i for i, x in enumerate(self.files)}              # :61
        self.device = dev
        self.cameras_host = cameras_host
        self.cameras = torch.from_numpy(cameras_host).to(dev)
        self.frames = frames_u8 if keep_frames else None
        parts = []
        for i in range(0, N, batch_size):
            chunk = frames_u8[i:i + batch_size].to(dev)
            flat = _frames_for_encode(chunk[None], codebook_model.config.image_size)
            parts.append(codebook_model.encode(flat)[-1].to(torch.int32))
        self.codes = torch.cat(parts).contiguous()                            # [N,t,t]

    def __len__(self):
        return len(self.files)                                                # :67-68

    def index(self, name) -> int:
        return self._lookup[name]

    def __getitem__(self, name):
        """SceneLookup.__getitem__ (:63-65) with the frame's bank index in the image loader's place: (camera [7] on the host, index)"""
        idx = self._lookup[name]
        return self.cameras_host[idx], idx

    def nearest(self, cameras, k: int):
        """the ``k`` bank views nearest to each camera [Q,7] (device): int32 [Q,k], ascending distance, ties to the lowest index"""
        cameras = torch.as_tensor(cameras, dtype=torch.float32).to(self.device)
        return ops.camera_knn(self.cameras, cameras.reshape(-1, 7), k, POS_WEIGHT)

    def gather(self, idx):
        """idx int [B,C] -> (codes int32 [B,C,t,t], cameras fp32 [B,C,7]) on the device"""
        idx = torch.as_tensor(idx).to(self.device).long()
        return self.codes[idx], self.cameras[idx]

    def frames_at(self, idx):
        """idx int [B,C] -> frames uint8 [B,C,H,W,3] on the device (needs ``keep_frames``)"""
        if self.frames is None:
            raise RuntimeError('SceneBank was built with keep_frames=False: it holds codes, not pixels')
        idx = torch.as_tensor(idx).long()
        return self.frames[idx.to(self.frames.device)].to(self.device)
