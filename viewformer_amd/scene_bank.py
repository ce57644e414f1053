"""Scene bank of the 7-Scenes localization evaluator: one scene's training views, encoded ONCE and kept on the GPU.

The reference's ``SceneLookup`` (viewformer/evaluate/evaluate_sevenscenes.py:48-68) keeps the training cameras, file names and image
loaders of a scene on the host; every query then stacks 19 context frames, uploads them and runs them through the encoder again
(:192-197, :240-244).  Codes are a pure function of the frame (the encoder is batch-invariant), so the bank encodes the scene's frames
once, in chunks, and keeps ``codes`` int32 [N,t,t] and ``cameras`` fp32 [N,7] on the device: a query's context is a gather, and the
pose refinement's search over every training camera (``compute_camera_distances`` + ``tf.argsort``, :188-189) is one kernel
(``ops.camera_knn``) on the stream.  The codes also answer "which training photos look like this one" (``similar``: ``ops.code_knn`` over
the codebook's distance table), which is what the evaluator's ``match_map`` holds and the reference reads from an outside retrieval
system's file (:71-77).  File names and the name -> index map of ``SceneLookup.__getitem__`` stay on the host.  Reading
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
        self.codebook_model = codebook_model                                  # similar(): its code distances, and its encoder for query images
        self._batch_size = batch_size
        self.cameras_host = cameras_host
        self.cameras = torch.from_numpy(cameras_host).to(dev)
        self.frames = frames_u8 if keep_frames else None
        self.codes = self._encode(frames_u8)                                  # [N,t,t]

    def _encode(self, frames_u8):
        """frames uint8 [n,H,W,3] (host or device) -> codes int32 [n,t,t] on the device, ``batch_size`` frames per encoder call"""
        parts = []
        for i in range(0, frames_u8.shape[0], self._batch_size):
            chunk = frames_u8[i:i + self._batch_size].to(self.device)
            flat = _frames_for_encode(chunk[None], self.codebook_model.config.image_size)
            parts.append(self.codebook_model.encode(flat)[-1].to(torch.int32))
        return torch.cat(parts).contiguous()

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

    def similar(self, codes=None, images=None, k: int = 1, window: int = 0, exclude=None, return_dist: bool = False):
        """the ``k`` bank views that look most like each query photo, given as exactly one of ``codes`` (int [Q,t,t]) and ``images``
        (uint8 [Q,H,W,3], encoded as the bank encodes its own frames): int32 [Q,k], nearest first, ties to the lowest index, in the
        code distance of ``ops.code_knn`` (``window=0``: the squared L2 distance of the quantised latent maps; ``window`` > 0 lets every
        query token find its partner up to that many tokens away).  ``exclude``: None or one bank index per query (-1: none) that the
        query must not return — a bank frame searching for its own neighbours.  ``return_dist`` adds the distances fp32 [Q,k]."""
        if (codes is None) == (images is None):
            raise ValueError('SceneBank.similar takes exactly one of codes and images')
        if images is not None:
            images = torch.as_tensor(images)
            if images.dim() != 4 or images.dtype != torch.uint8:
                raise ValueError(f'SceneBank.similar: images uint8 [Q,H,W,3] expected, got {tuple(images.shape)} {images.dtype}')
            codes = self._encode(images)
        else:
            codes = torch.as_tensor(codes)
            if codes.dim() != 3 or codes.is_floating_point() or tuple(codes.shape[1:]) != tuple(self.codes.shape[1:]):
                raise ValueError(f'SceneBank.similar: integer codes [Q,{self.codes.shape[1]},{self.codes.shape[2]}] expected, got '
                                 f'{tuple(codes.shape)} {codes.dtype}')
            codes = codes.to(self.device).to(torch.int32)
        return ops.code_knn(self.codes, codes, self.codebook_model.code_distances(), k, window, exclude, return_dist)

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
