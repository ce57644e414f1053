"""Thin tensor-level wrappers over the C-ABI (include/vf_hip.h).

PyTorch is used for device memory and the stream handle only: every wrapper hands raw
device pointers to libvf_hip.so and launches on torch's current HIP stream.  Nothing here
computes with torch ops, and nothing falls back to them.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import VfIgemmArgs, check

MODE_GEMM, MODE_CONV3_S1, MODE_CONV3_S2PAD, MODE_CONV3_UP2 = 0, 1, 2, 3
EPI_NONE, EPI_GELU, EPI_GELU_BWD, EPI_GELU_DUAL = 0, 1, 2, 3


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _chk(t, dtype=torch.float32, name='tensor'):
    if not t.is_cuda:
        raise _lib.VfError(f'{name} must live on the GPU (no CPU fallback for the hot path)')
    if t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')
    return t


def _f32(t, name='tensor'):
    return _chk(t, torch.float32, name)


# ------------------------------------------------------------------ weight packing
def packed_floats(K, N, taps=1):
    return int(_lib.load().vf_igemm_packed_floats(K, N, taps))


def pack(src, K, N, taps, sk, sn, st, batch=1, src_bstride=0, out=None):
    """pack element (tap,k,n) = src[tap*st + k*sk + n*sn] into the fragment-major layout"""
    lib = _lib.load()
    n = packed_floats(K, N, taps)
    if out is None:
        out = torch.empty(batch * n, dtype=torch.float32, device=src.device)
    check(lib.vf_igemm_pack_f32(_p(_f32(src)), _p(out), K, N, taps, sk, sn, st, batch, src_bstride, _stream()),
          'vf_igemm_pack_f32')
    return out


def pack_conv_oihw(w):
    """torch Conv2d weight [Cout][Cin][kh][kw], kh=kw in {1,3}"""
    w = _f32(w).contiguous()
    cout, cin, kh, kw = w.shape
    taps = kh * kw
    return pack(w, cin, cout, taps, sk=taps, sn=cin * taps, st=1)


def pack_dense_kn(w):
    """Conv1D weight [nx][nf] (x @ W)"""
    w = _f32(w).contiguous()
    k, n = w.shape
    return pack(w, k, n, 1, sk=n, sn=1, st=0)


def pack_dense_nk(w, n_rows=None):
    """transposed weight [N][K] (x @ W^T), optionally only the first n_rows rows"""
    w = _f32(w).contiguous()
    n, k = w.shape
    n = n if n_rows is None else n_rows
    return pack(w, k, n, 1, sk=1, sn=k, st=0)


# one row per arm: the library's size and pack symbols, the packing's dtype, what the pack symbol takes behind the two strides
_DENSE_PACK = {'bf16': ('vf_gemm_bf16_packed_elems', 'vf_gemm_bf16_pack', torch.bfloat16, (1, 0)),
               'x6': ('vf_gemm_x6_packed_elems', 'vf_gemm_x6_pack', torch.bfloat16, ()),
               'x3h': ('vf_gemm_x3h_packed_elems', 'vf_gemm_x3h_pack', torch.float16, ())}
_CONV3_PACK = {'bf16': ('vf_conv3_bf16_packed_elems', 'vf_conv3_bf16_pack', torch.bfloat16),
               'x6': ('vf_conv3_x6_packed_elems', 'vf_conv3_x6_pack', torch.bfloat16),
               'x3h': ('vf_conv3_x3h_packed_elems', 'vf_conv3_x3h_pack', torch.float16)}


def _pack_dense(arm, w, transposed, n_rows=None):
    """w = [K][N] (x @ W), or ``transposed`` [N][K] (x @ W^T), optionally only its first n_rows rows -> the arm's packing"""
    size, pack_fn, dtype, tail = _DENSE_PACK[arm]
    lib = _lib.load()
    w = _f32(w).contiguous()
    n, k = w.shape if transposed else w.shape[::-1]
    n = n if n_rows is None else n_rows
    out = torch.empty(int(getattr(lib, size)(k, n)), dtype=dtype, device=w.device)
    check(getattr(lib, pack_fn)(_p(w), _p(out), k, n, *((1, k) if transposed else (n, 1)), *tail, _stream()), pack_fn)
    return out


def _pack_conv3(arm, w_oihw):
    size, pack_fn, dtype = _CONV3_PACK[arm]
    lib = _lib.load()
    w = _f32(w_oihw).contiguous()
    cout, cin = w.shape[:2]
    out = torch.empty(int(getattr(lib, size)(cin, cout)), dtype=dtype, device=w.device)
    check(getattr(lib, pack_fn)(_p(w), _p(out), cin, cout, _stream()), pack_fn)
    return out


# ------------------------------------------------------------------ implicit GEMM
def pack_dense_kn_bf16(w):
    """Conv1D weight [nx][nf] -> bf16 fragment packing for vf_gemm_bf16"""
    return _pack_dense('bf16', w, False)


def pack_bf16_multi(items):
    """many bf16 packings in one launch.  ``items`` = [(w fp32 [rows][cols] contiguous, transposed, out)]: transposed False packs w as
    [K = rows][N = cols] (pack_dense_kn_bf16), True as the [N = rows][K = cols] operand (pack_dense_nk_bf16); ``out`` = the bf16 buffer to
    fill (vf_gemm_bf16_packed_elems(K, N)).  Returns a closure that re-runs the same launch (descriptors stay on the device)."""
    import numpy as np
    lib = _lib.load()
    dt = np.dtype([('src', '<u8'), ('dst', '<u8'), ('K', '<i4'), ('N', '<i4'), ('sk', '<i8'), ('sn', '<i8')])
    assert dt.itemsize == _lib.PACK_DESC_BYTES
    a = np.zeros(len(items), dtype=dt)
    for i, (w, tr, out) in enumerate(items):
        _f32(w); _chk(out, torch.bfloat16)
        assert w.is_contiguous() and w.dim() == 2
        r, c = w.shape
        K, N, sk, sn = (c, r, 1, c) if tr else (r, c, c, 1)
        assert out.numel() >= int(lib.vf_gemm_bf16_packed_elems(K, N))
        a[i] = (w.data_ptr(), out.data_ptr(), K, N, sk, sn)
    descs = torch.from_numpy(a.view(np.uint8).copy()).to(items[0][0].device)
    n = len(items)

    def run(first=0, count=None):
        """re-pack items [first, first + count) (default: all of them)"""
        count = n - first if count is None else count
        if count <= 0:
            return
        assert 0 <= first and first + count <= n
        check(lib.vf_gemm_bf16_pack_multi(descs.data_ptr() + first * _lib.PACK_DESC_BYTES, count, _stream()), 'vf_gemm_bf16_pack_multi')
    run()
    return run


def pack_dense_nk_bf16(w, n_rows=None):
    """transposed weight [N][K] (x @ W^T; tied LM head, 1x1 conv [Cout][Cin]) -> bf16 packing"""
    return _pack_dense('bf16', w, True, n_rows)


def pack_conv3_bf16(w_oihw):
    return _pack_conv3('bf16', w_oihw)


def pack_conv3_x6(w_oihw):
    """OIHW fp32 3x3 weight -> three fragment-packed bf16 planes (exact split w = h + m + l) for vf_conv3_halo_x6"""
    return _pack_conv3('x6', w_oihw)


def pack_conv3_x3h(w_oihw):
    """OIHW fp32 3x3 weight -> two fragment-packed f16 planes of w * S (S a power of two, 1/S stored behind them) for
    vf_conv3_halo_x3h"""
    return _pack_conv3('x3h', w_oihw)


def pack_dense_kn_x6(w):
    """Conv1D weight [nx][nf] -> 3-plane split packing for vf_gemm_x6"""
    return _pack_dense('x6', w, False)


def pack_dense_nk_x6(w, n_rows=None):
    """transposed weight [N][K] (x @ W^T; tied LM head, 1x1 conv [Cout][Cin]) -> 3-plane split packing"""
    return _pack_dense('x6', w, True, n_rows)


def pack_dense_kn_x3h(w):
    """Conv1D weight [nx][nf] -> two-plane split-fp16 packing (w * S, 1/S behind the planes) for vf_gemm_x3h"""
    return _pack_dense('x3h', w, False)


def pack_dense_nk_x3h(w, n_rows=None):
    """transposed weight [N][K] (x @ W^T; tied LM head, 1x1 conv [Cout][Cin]) -> two-plane split-fp16 packing"""
    return _pack_dense('x3h', w, True, n_rows)


def gemm_x6_splitk(x, w_packed, M, Cin, Cout, dst, splits, lda=None, accumulate=True):
    """dst[M][Cout] (+)= x @ W with the reduction split over ``splits`` workgroup groups (deterministic: slabs summed in order);
    for GEMMs whose output has too few 128x128 tiles to fill the chip but a long reduction (the training step's dW)"""
    lib = _lib.load()
    slabs = torch.empty((splits, M, Cout), dtype=torch.float32, device=x.device)
    igemm(x, w_packed, M, Cin, Cout, slabs, lda=lda, x6=True, split_k=splits, stride_out=M * Cout)
    check(lib.vf_sum_slabs_f32(_p(slabs), splits, M * Cout, M * Cout, _p(_f32(dst)), 1 if accumulate else 0, _stream()),
          'vf_sum_slabs_f32')
    return dst


def conv3_x6_supported(mode, Cin, Cout, Hout, Wout):
    """shape rules of vf_conv3_halo_x6 (host-side mirror so callers can pick the packing up front)"""
    if mode not in (MODE_CONV3_S1, MODE_CONV3_UP2, MODE_CONV3_S2PAD) or Cin % 32 or Cout % 128:
        return False
    return (Hout % 8 == 0 and Wout % 16 == 0) or (mode == MODE_CONV3_S1 and Hout == 8 and Wout == 8)


def conv3_x3h_supported(mode, Cin, Cout, Hout, Wout):
    """shape rules of vf_conv3_halo_x3h: the x6 kernel's, plus the 16x16 -> 8x8 stride-2 convolution (two images per tile)"""
    if mode == MODE_CONV3_S2PAD and Hout == 8 and Wout == 8 and Cin % 32 == 0 and Cout % 128 == 0:
        return True
    return conv3_x6_supported(mode, Cin, Cout, Hout, Wout)


# the codec's call sites (vqgan.py, vqgan_train.py, lpips.py) name a launch's arithmetic ("arm"); igemm takes it as boolean keywords
ARM_KW = {'f32': {}, 'x6': dict(x6=True), 'x3h': dict(x3h=True), 'bf16': dict(bf16=True)}


def conv3_arm(mode, Cin, Cout, Hout, Wout, activations=False, res=False):
    """the arm of a 3x3 convolution whose weight is packed for the launch (codebook trainer, LPIPS): 'small' = the small-cout kernel
    (conv3_small_cout, no residual), else 'x6' where conv3_x6_supported — 'x3h' on top for forward ``activations`` (O(1) magnitudes;
    gradients, ~1e-6, stay on x6, which has no range condition: DESIGN.md 4) — else the native 'f32'"""
    if not res and conv3_small_cout_supported(mode, Cin, Cout, Hout, Wout):
        return 'small'
    if conv3_x6_supported(mode, Cin, Cout, Hout, Wout):
        return 'x3h' if activations else 'x6'
    return 'f32'


def pack_conv3(arm, w_oihw):
    """3x3 OIHW weight -> the packing igemm(**ARM_KW[arm]) reads"""
    return {'f32': pack_conv_oihw, 'x6': pack_conv3_x6, 'x3h': pack_conv3_x3h, 'bf16': pack_conv3_bf16}[arm](w_oihw)


def pack_dense_nk_arm(arm, w, n_rows=None):
    """transposed weight [N][K] -> the packing igemm(**ARM_KW[arm]) reads"""
    return {'f32': pack_dense_nk, 'x6': pack_dense_nk_x6, 'x3h': pack_dense_nk_x3h, 'bf16': pack_dense_nk_bf16}[arm](w, n_rows)


def pack_dense(arm, w, transposed=False, n_rows=None):
    """w [K][N] for x @ W, or ``transposed`` [N][K] (its first n_rows rows) for x @ W^T -> the packing igemm(**ARM_KW[arm]) reads"""
    fn = globals()['pack_dense_' + ('nk' if transposed else 'kn') + ('' if arm == 'f32' else '_' + arm)]
    return fn(w) if n_rows is None else fn(w, n_rows=n_rows)


def gemm_bf16_splitk(x, w_packed, M, Cin, Cout, dst, splits, lda=None, accumulate=True):
    """dst[M][Cout] (+)= x @ W on the bf16 arm with the reduction split over ``splits`` slabs: the split-K of a weight-gradient GEMM
    (few output tiles, a reduction of tens of thousands of rows) expressed as a BATCHED launch of vf_gemm_bf16 — batch entry s
    reads columns [s Cin/splits, (s+1) Cin/splits) of x and the matching 64-deep chunk range of the chunk-major packing — followed by
    the fixed-order slab sum (deterministic).  Cin / splits must be a multiple of 64 (the packing's chunk)."""
    lib = _lib.load()
    ks = Cin // splits
    if splits < 1 or ks * splits != Cin or ks % 64:
        raise _lib.VfError(f'gemm_bf16_splitk: Cin = {Cin} does not split into {splits} ranges of whole 64-deep chunks')
    nb = (Cout + 127) // 128
    slabs = torch.empty((splits, M, Cout), dtype=torch.float32, device=x.device)
    igemm(x, w_packed, M, ks, Cout, slabs, lda=Cin if lda is None else lda, bf16=True, batch=splits, stride_x=ks,
          stride_w=(ks // 64) * nb * 64 * 128, stride_out=M * Cout)
    check(lib.vf_sum_slabs_f32(_p(slabs), splits, M * Cout, M * Cout, _p(_f32(dst)), 1 if accumulate else 0, _stream()),
          'vf_sum_slabs_f32')
    return dst


TN_TARGET_WORKGROUPS = 256             # row-range splits of the weight-gradient GEMM: tiles x splits ~ one workgroup per CU when the launch has the machine to
TN_TARGET_WORKGROUPS_BESIDE = 192      # itself; ~ three quarters of the CUs when it is issued beside another GEMM (the trainer's second stream: the dX GEMM of the
                                       # same layer runs on the main stream).  Every split writes an fp32 slab that vf_sum_slabs_f32 folds.  Round 6, in-process
                                       # alternation of the training step over the "beside" value: 256 (7 splits of the 36-tile layers) 19.72 ms, 224 (6) 19.71,
                                       # 208 / 192 (5) 19.47-19.49, 176 (4) 19.65, 128 19.85 — five slabs instead of seven are 29 % less slab traffic and the
                                       # parallelism they give up was not there to have (profiles/r6_small_kernels.txt).  Alone (the serialised step bench.py
                                       # instruments for the roofline section) the full-machine split is the faster one.


def gemm_tn_bf16_supported(x, M, K, N):
    return x.dtype == torch.bfloat16 and gemm_tn_bf16_shape_ok(M, K, N)


def gemm_tn_bf16_shape_ok(M, K, N):
    """shapes vf_gemm_tn_bf16 takes (csrc/gemm_tn_bf16.hip): 256-wide tiles of dW, 64-row chunks, 32-bit offsets into x"""
    return K % 256 == 0 and N % 256 == 0 and M % 64 == 0 and M * K * 2 < 2 ** 31


def gemm_g256_shape_ok(M, K, N):
    """shapes the 256-tile LDS-DMA bf16 GEMM takes (csrc/gemm_bf16_g256.hip: vf_gemm_bf16_g256_launch) — the only kernel behind the fused
    epilogues EPI_GELU_DUAL, EPI_GELU_BWD with a bf16 pre-activation, and the fused output dropout"""
    return N % 256 == 0 and K % 64 == 0 and M >= 256 and M * K * 2 < 2 ** 31 and K * N * 2 < 2 ** 31


def gemm_drop_supported(M, K, N, row0=0):
    """the fused output dropout of vf_gemm_bf16 (igemm(drop=...)): 256-tile shapes, 32-bit mask group indices"""
    return gemm_g256_shape_ok(M, K, N) and row0 % 4 == 0 and ((M + row0 + 3) // 4) * N < 2 ** 32


def gemm_tn_bf16(x16, dy, M, K, N, dw, db=None, accumulate=True, beside_another_gemm=False):
    """dw[K][N] (+)= x16^T @ dy and db[N] (+)= column sums of dy, straight from the row-major bf16 activation x16 [M][K] and the fp32
    gradient dy [M][N] (csrc/gemm_tn_bf16.hip): split-K slabs folded in slab order (deterministic)."""
    lib = _lib.load()
    _chk(x16, torch.bfloat16, 'x16')
    tiles = (K // 256) * (N // 256)
    target = TN_TARGET_WORKGROUPS_BESIDE if beside_another_gemm else TN_TARGET_WORKGROUPS
    splits = max(1, min(M // 64, target // tiles if tiles <= target else 1))
    # one array of `splits` records (weight slab | bias slab): where the gradient buffer holds the bias right behind the weight (the trainer's
    # flat buffer does), ONE slab sum folds both
    rec = K * N + (N if db is not None else 0)
    ws = torch.empty((splits, rec), dtype=torch.float32, device=dy.device)
    y16 = dy.dtype == torch.bfloat16
    check(lib.vf_gemm_tn_bf16(_p(x16), x16.stride(0), _p(dy if y16 else _f32(dy)), 1 if y16 else 0, dy.stride(0), M, K, N, splits, _p(ws),
                              ws.data_ptr() + K * N * 4 if db is not None else None, rec, _stream()), 'vf_gemm_tn_bf16')
    acc = 1 if accumulate else 0
    _f32(dw)
    if db is not None and _f32(db).data_ptr() == dw.data_ptr() + K * N * 4 and dw.is_contiguous():
        check(lib.vf_sum_slabs_f32(_p(ws), splits, rec, rec, _p(dw), acc, _stream()), 'vf_sum_slabs_f32')
    else:
        check(lib.vf_sum_slabs_f32(_p(ws), splits, rec, K * N, _p(dw), acc, _stream()), 'vf_sum_slabs_f32')
        if db is not None:
            check(lib.vf_sum_slabs_f32(ws.data_ptr() + K * N * 4, splits, rec, N, _p(db), acc, _stream()), 'vf_sum_slabs_f32')
    return dw


def igemm(x, w_packed, M, Cin, Cout, out, bias=None, res=None, mode=MODE_GEMM, epilogue=EPI_NONE,
          pro=None, pro_swish=False, pro_rows_per_img=0, Hin=0, Win=0, Hout=0, Wout=0,
          lda=None, ldc=None, ldr=None, batch=1, stride_x=0, stride_w=0, stride_out=0, stride_res=0, bf16=False, x6=False, gn_part=None, split_k=0,
          x3h=False, a16=False, o16=False, out_aux=None, res16=False, drop=None, gelu_grad=False):
    """``bf16=True``: w_packed is a bf16 packing (pack_*_bf16) and the launch goes to the bf16-MFMA arm
    (vf_gemm_bf16 / vf_conv3_halo_bf16); unsupported shapes raise (no silent fallback).
    ``x6=True``: w_packed is the 3-plane split packing (pack_conv3_x6) and the launch goes to the fp32-equivalent
    split-bf16 kernel (vf_conv3_halo_x6).
    ``gn_part``: fp32 [Nimg][halo_gn_slots(Hout, Wout)][32][2] buffer that receives the GroupNorm partial statistics of the
    output (halo kernels only; reduce with groupnorm_finalize).
    ``out_aux`` (with ``epilogue=EPI_GELU_DUAL``, bf16 arm, bf16 x, fp32 or bf16 out): bf16 [M][ldc] that receives gelu(out).
    ``res16`` (with ``epilogue=EPI_GELU_BWD``): the pre-activation behind ``res`` was saved as bf16.
    ``gelu_grad`` (round 6, 256-tile shapes): with ``EPI_GELU_DUAL`` and bf16 out, ``out`` receives gelu'(x @ W + b) instead of the pre-activation;
    with ``EPI_GELU_BWD`` and ``res16``, ``res`` holds that saved derivative and the epilogue multiplies by it instead of evaluating gelu' again.
    ``drop`` = (rate, seed, site), bf16 arm with bf16 x and fp32 out only: the training step's output dropout in the epilogue, before the
    residual joins (vf_igemm_args.drop_rate; the masks of train_ops.dropout_add with cols = Cout).  Shapes outside the 256-tile kernel
    raise 'unsupported' (callers run the GEMM, then dropout_add)."""
    lib = _lib.load()
    if not 0 <= M < 2 ** 31 or max(Cin, Cout, Hin, Win, Hout, Wout, batch) >= 2 ** 31:
        # vf_igemm_args carries 32-bit row / channel counts (byte offsets inside the kernels are 64-bit): refuse instead of wrapping
        raise _lib.VfError(f'igemm: M = {M} rows do not fit the int32 fields of vf_igemm_args — split the launch '
                           '(VQGAN(max_images_per_call=...))')
    a = VfIgemmArgs()
    a.x = x.data_ptr()
    a.w_packed = w_packed.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.res = res.data_ptr() if res is not None else None
    a.out = out.data_ptr()
    if out_aux is not None:
        _chk(out_aux, torch.bfloat16, 'out_aux')
        if out_aux.shape != out.shape or not (out_aux.is_contiguous() or out_aux.stride() == out.stride()):
            raise _lib.VfError('out_aux must have the shape and row stride of out')
        a.out_aux = out_aux.data_ptr()
    if pro is not None:
        mean_c, scale_c, beta = pro
        a.pro_mean, a.pro_scale, a.pro_beta = mean_c.data_ptr(), scale_c.data_ptr(), beta.data_ptr()
    a.pro_swish = 1 if pro_swish else 0
    a.pro_rows_per_img = pro_rows_per_img
    a.mode, a.epilogue = mode, epilogue
    a.M, a.Cin, a.Cout = M, Cin, Cout
    a.Hin, a.Win, a.Hout, a.Wout = Hin, Win, Hout, Wout
    a.lda = Cin if lda is None else lda
    a.ldc = Cout if ldc is None else ldc
    a.ldr = (Cout if ldr is None else ldr)
    a.batch = batch
    a.stride_x, a.stride_w, a.stride_out, a.stride_res = stride_x, stride_w, stride_out, stride_res
    a.reserved0 = split_k                     # vf_gemm_x6: number of split-K slabs written at out + s*stride_out
    if gn_part is not None:
        a.gn_part = _f32(gn_part).data_ptr()
        a.gn_slots = gn_part.shape[1]
    conv16 = False
    if a16 or o16:                            # bf16 activations in / out: the bf16 arm only (dtype flags in reserved0)
        if not bf16 or mode not in (MODE_GEMM, MODE_CONV3_S1, MODE_CONV3_UP2):
            raise _lib.VfError('a16 / o16 need bf16=True and a GEMM or 3x3 stride-1 / upsample convolution')
        _chk(x, torch.bfloat16 if a16 else torch.float32, 'x')
        _chk(out, torch.bfloat16 if o16 else torch.float32, 'out')
        a.reserved0 = (1 if a16 else 0) | (2 if o16 else 0)
        conv16 = mode != MODE_GEMM
        if conv16:                            # vf_conv3_halo_bf16: bf16 out means a bf16 residual too (the same activation stream)
            if a16 and not o16:
                raise _lib.VfError('the bf16 convolution takes bf16 activations in only together with bf16 out')
            if res is not None:
                _chk(res, torch.bfloat16 if o16 else torch.float32, 'res')
    if drop is not None and drop[0]:
        if not (bf16 and a16 and not o16 and mode == MODE_GEMM and epilogue == EPI_NONE):
            raise _lib.VfError('drop needs the bf16 GEMM with bf16 x, fp32 out and no epilogue function')
        a.drop_rate, a.drop_seed, a.drop_site = float(drop[0]), int(drop[1]) & 0xFFFFFFFF, int(drop[2])
        a.drop_row0 = int(drop[3]) if len(drop) > 3 else 0          # first row's index in the global batch (data-parallel step)
    if res16:
        if not (a16 and o16 and epilogue == EPI_GELU_BWD and res is not None):
            raise _lib.VfError('res16 is the bf16 pre-activation of EPI_GELU_BWD (bf16 in, bf16 out)')
        _chk(res, torch.bfloat16, 'res')
        a.reserved0 |= 4
    if gelu_grad:
        if not ((epilogue == EPI_GELU_DUAL and a16 and o16) or (epilogue == EPI_GELU_BWD and res16)):
            raise _lib.VfError('gelu_grad: EPI_GELU_DUAL with bf16 in / out, or EPI_GELU_BWD with res16')
        a.reserved0 |= 8
    for t in ((None if a16 else x), (None if o16 else out), bias, (None if (res16 or conv16) else res)):
        if t is not None:
            _f32(t)
    if x3h:                                   # w_packed = pack_conv3_x3h / pack_dense_*_x3h: the 3-product split-fp16 kernels
        _chk(w_packed, torch.float16, 'w_packed')
        if mode == MODE_GEMM:
            check(lib.vf_gemm_x3h(ctypes.byref(a), _stream()), 'vf_gemm_x3h')
        else:
            check(lib.vf_conv3_halo_x3h(ctypes.byref(a), _stream()), 'vf_conv3_halo_x3h')
        return out
    if x6:
        _chk(w_packed, torch.bfloat16, 'w_packed')
        if mode == MODE_GEMM:
            check(lib.vf_gemm_x6(ctypes.byref(a), _stream()), 'vf_gemm_x6')
        else:
            check(lib.vf_conv3_halo_x6(ctypes.byref(a), _stream()), 'vf_conv3_halo_x6')
        return out
    if bf16:
        _chk(w_packed, torch.bfloat16, 'w_packed')
        if mode == MODE_GEMM:
            check(lib.vf_gemm_bf16(ctypes.byref(a), _stream()), 'vf_gemm_bf16')
        else:
            check(lib.vf_conv3_halo_bf16(ctypes.byref(a), _stream()), 'vf_conv3_halo_bf16')
        return out
    _f32(w_packed)
    check(lib.vf_igemm_f32(ctypes.byref(a), _stream()), 'vf_igemm_f32')
    return out


def conv3_small_cout_supported(mode, Cin, Cout, H, W):
    # the kernel keeps ALL weights in LDS (Cin / 32 x 4608 B, at most 96 KiB: Cin <= 672); wider inputs take the implicit-GEMM path
    return mode == MODE_CONV3_S1 and 1 <= Cout <= 4 and Cin % 32 == 0 and Cin // 32 * 4608 <= 96 * 1024 and H % 8 == 0 and W % 32 == 0


def conv3_small_cout(x, w_oihw, bias, n_img, H, W, Cin, Cout, pro=None, pro_swish=True, out=None):
    """3x3 conv to <= 4 channels (decoder conv_out) with the fused GroupNorm(+swish) prologue; x NHWC rows, fp32 or bf16"""
    lib = _lib.load()
    if out is None:
        out = torch.empty((n_img * H * W, Cout), dtype=torch.float32, device=x.device)
    pm, ps, pb = (None, None, None) if pro is None else pro
    x16 = x.dtype == torch.bfloat16
    check(lib.vf_conv3_small_cout_f32(_p(x if x16 else _f32(x)), _p(_f32(w_oihw)), _p(_f32(bias)) if bias is not None else None,
                                      _p(pm) if pm is not None else None, _p(ps) if ps is not None else None,
                                      _p(pb) if pb is not None else None, 1 if pro_swish else 0, _p(out), n_img, H, W, Cin, Cout,
                                      1 if x16 else 0, _stream()), 'vf_conv3_small_cout_f32')
    return out


def pack_conv_in_x3h(w_oihw):
    """encoder.conv_in weight [Cout][3][3][3] -> split-fp16 packing for the matrix-pipe form of conv_in (Cout % 128 == 0)"""
    lib = _lib.load()
    w = _f32(w_oihw).contiguous()
    out = torch.empty(int(lib.vf_conv_in_x3h_packed_elems(w.shape[0])), dtype=torch.float16, device=w.device)
    check(lib.vf_conv_in_x3h_pack(_p(w), _p(out), w.shape[0], _stream()), 'vf_conv_in_x3h_pack')
    return out


def conv_in_x3h_supported(H, W, Cout):
    return H % 8 == 0 and W % 16 == 0 and Cout % 128 == 0


def conv_in(img, w_oihw, bias, n_img, H, W, Cout, out=None, wp3h=None, gn_part=None):
    """img: uint8 NHWC [n,H,W,3] (TF evaluator entry) or float32 NHWC already in [-1,1].  ``wp3h`` (pack_conv_in_x3h): run on the
    matrix pipe (fp32-equivalent x3h arithmetic), optionally emitting the GroupNorm partial statistics of the output (gn_part)"""
    lib = _lib.load()
    if out is None:
        out = torch.empty((n_img, H, W, Cout), dtype=torch.float32, device=img.device)
    if img.dtype == torch.uint8:
        u8, f32 = _p(_chk(img, torch.uint8)), None
    else:
        u8, f32 = None, _p(_f32(img))
    if wp3h is not None:
        _chk(wp3h, torch.float16, 'wp3h')
        check(lib.vf_conv_in_x3h(u8, f32, _p(wp3h), _p(bias), _p(out), _p(gn_part) if gn_part is not None else None,
                                 gn_part.shape[1] if gn_part is not None else 0, n_img, H, W, Cout, _stream()), 'vf_conv_in_x3h')
        return out
    if gn_part is not None:
        raise _lib.VfError('conv_in: fused GroupNorm statistics need the x3h form (wp3h)')
    check(lib.vf_conv_in_u8_f32(u8, f32, _p(_f32(w_oihw)), _p(bias), _p(out), n_img, H, W, Cout, _stream()),
          'vf_conv_in_u8_f32')
    return out


# ------------------------------------------------------------------ GroupNorm
def groupnorm_stats(x, gamma, n_img, HW, C, groups=32, eps=1e-6):
    lib = _lib.load()
    mean_c = torch.empty((n_img, C), dtype=torch.float32, device=x.device)
    scale_c = torch.empty((n_img, C), dtype=torch.float32, device=x.device)
    ws = torch.empty(int(lib.vf_groupnorm_workspace_bytes(n_img, HW, C)), dtype=torch.uint8, device=x.device)
    check(lib.vf_groupnorm_stats_f32(_p(_f32(x)), _p(_f32(gamma)), n_img, HW, C, groups, eps, _p(mean_c), _p(scale_c),
                                     _p(ws), _stream()), 'vf_groupnorm_stats_f32')
    return mean_c, scale_c


def halo_gn_slots(Hout, Wout):
    """partial-statistics slots per image the halo conv kernels write for an Hout x Wout output (0 = not a halo shape)"""
    return int(_lib.load().vf_conv3_halo_gn_slots(Hout, Wout))


def new_gn_part(n_img, Hout, Wout, device):
    """buffer for igemm(..., gn_part=...): every slot is written by the producing conv, no initialisation needed"""
    return torch.empty((n_img, halo_gn_slots(Hout, Wout), 32, 2), dtype=torch.float32, device=device)


def groupnorm_finalize(part, gamma, n_img, HW, C, groups=32, eps=1e-6):
    """second half of groupnorm_stats from partials written by a conv's fused epilogue (the activation is not re-read)"""
    lib = _lib.load()
    mean_c = torch.empty((n_img, C), dtype=torch.float32, device=part.device)
    scale_c = torch.empty((n_img, C), dtype=torch.float32, device=part.device)
    check(lib.vf_groupnorm_finalize_f32(_p(_f32(part)), _p(_f32(gamma)), n_img, HW, C, groups, part.shape[1], eps,
                                        _p(mean_c), _p(scale_c), _stream()), 'vf_groupnorm_finalize_f32')
    return mean_c, scale_c


def groupnorm_apply(x, mean_c, scale_c, beta, n_img, HW, C, swish, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(x)
    check(lib.vf_groupnorm_apply_f32(_p(_f32(x)), _p(mean_c), _p(scale_c), _p(_f32(beta)), _p(out), n_img, HW, C,
                                     1 if swish else 0, _stream()), 'vf_groupnorm_apply_f32')
    return out


# ------------------------------------------------------------------ codebook
def vq_pack_codebook(E):
    lib = _lib.load()
    E = _f32(E).contiguous()
    D, Kc = E.shape
    out = torch.empty(int(lib.vf_vq_packed_floats(D, Kc)), dtype=torch.float32, device=E.device)
    check(lib.vf_vq_pack_codebook_f32(_p(E), _p(out), D, Kc, _stream()), 'vf_vq_pack_codebook_f32')
    e_sq = torch.empty(Kc, dtype=torch.float32, device=E.device)
    check(lib.vf_colsumsq_f32(_p(E), _p(e_sq), D, Kc, _stream()), 'vf_colsumsq_f32')
    return out, e_sq


def vq_argmin(z_rows, E_packed, e_sq, D, Kc):
    lib = _lib.load()
    z_rows = _f32(z_rows)
    M = z_rows.numel() // D
    idx = torch.empty(M, dtype=torch.int64, device=z_rows.device)
    check(lib.vf_vq_argmin_f32(_p(z_rows), _p(E_packed), _p(e_sq), M, D, Kc, _p(idx), _stream()), 'vf_vq_argmin_f32')
    return idx


def vq_filter_supported(D, Kc):
    """shape rules of the filtered lookup (vf_vq_argmin_filtered_f32): otherwise call vq_argmin (same result, f32 MFMA)"""
    return int(_lib.load().vf_vq_filter_packed_bytes(D, Kc)) > 0


def vq_filter_pack(E):
    """reference ``embeddings`` [D][Kc] -> the filtered lookup's blob (fp16 fragment tiles, fp32 transpose, e_sq, window constants)"""
    lib = _lib.load()
    E = _f32(E).contiguous()
    D, Kc = E.shape
    n = int(lib.vf_vq_filter_packed_bytes(D, Kc))
    if n == 0:
        raise _lib.VfError(f'vq_filter_pack: unsupported codebook shape D={D}, Kc={Kc} (need D == 256, Kc % 32 == 0, Kc <= 1024)')
    out = torch.empty(n, dtype=torch.uint8, device=E.device)
    check(lib.vf_vq_filter_pack(_p(E), _p(out), D, Kc, _stream()), 'vf_vq_filter_pack')
    return out


def vq_argmin_filtered(z_rows, blob, D, Kc, stats=None):
    """codebook lookup through the fp16 candidate filter + exact fp32 re-rank: the same indices as vq_argmin, bit for bit.
    ``stats``: optional zero-initialised int32[4] device tensor receiving (filter-certified rows, re-ranked rows, exact distance
    evaluations, fully scanned rows)"""
    lib = _lib.load()
    z_rows = _f32(z_rows)
    M = z_rows.numel() // D
    idx = torch.empty(M, dtype=torch.int64, device=z_rows.device)
    check(lib.vf_vq_argmin_filtered_f32(_p(z_rows), _p(_chk(blob, torch.uint8, 'blob')), M, D, Kc, _p(idx),
                                        _p(_chk(stats, torch.int32, 'stats')) if stats is not None else None, _stream()),
          'vf_vq_argmin_filtered_f32')
    return idx


def codebook_gather(E, idx, D, Kc):
    lib = _lib.load()
    idx = _chk(idx, torch.int64, 'codes').contiguous()
    M = idx.numel()
    out = torch.empty((M, D), dtype=torch.float32, device=idx.device)
    check(lib.vf_codebook_gather_f32(_p(_f32(E)), _p(idx), _p(out), M, D, Kc, _stream()), 'vf_codebook_gather_f32')
    return out


# ------------------------------------------------------------------ attention / transformer glue
def attn_blockcausal(q, k, v, out, B, H, T, L, ldq, ldk, ldv, ldo, scale=1.0, skip_masked=True, twin_view=-1, bf16=False, x6=False,
                     fp8=False):
    """``bf16`` / ``fp8``: the tolerance arms (bf16 or OCP e4m3 operands, fp32 softmax; csrc/attention_lp.hip, and for bf16 tensors with
    64-token views the LDS-DMA kernel of csrc/attention_dma.hip); ``x6``: fp32-equivalent; default: native f32 MFMA."""
    lib = _lib.load()
    if fp8:
        bf16 = True
    if x6:
        check(lib.vf_attn_blockcausal_x6(_p(_f32(q)), _p(_f32(k)), _p(_f32(v)), _p(_f32(out)), B, H, T, L, ldq, ldk, ldv,
                                         ldo, scale, 1 if skip_masked else 0, twin_view, _stream()),
              'vf_attn_blockcausal_x6')
        return out
    if bf16:
        o16 = out.dtype == torch.bfloat16          # bf16 output for a bf16-GEMM consumer (igemm(..., a16=True))
        i16 = q.dtype == torch.bfloat16            # bf16 q/k/v: the fused c_attn output written by its GEMM with o16=True
        for t in (q, k, v):
            _chk(t, torch.bfloat16 if i16 else torch.float32, 'q/k/v')
        fn = lib.vf_attn_blockcausal_fp8 if fp8 else lib.vf_attn_blockcausal_bf16_v2
        check(fn(_p(q), _p(k), _p(v), 1 if i16 else 0, _p(out if o16 else _f32(out)), 1 if o16 else 0, B, H, T, L,
                 ldq, ldk, ldv, ldo, scale, 1 if skip_masked else 0, twin_view, _stream()), 'vf_attn_blockcausal_lp')
        return out
    check(lib.vf_attn_blockcausal_f32(_p(_f32(q)), _p(_f32(k)), _p(_f32(v)), _p(_f32(out)), B, H, T, L, ldq, ldk, ldv,
                                      ldo, scale, 1 if skip_masked else 0, twin_view, _stream()),
          'vf_attn_blockcausal_f32')
    return out


def attn_prefix(q, k, v, kp, vp, out, B, H, C, N, L, ldq, ldk, ldv, ldkp, ldvp, prefix_stride, ldo, bf16=False, dh=64, ctx_len=None):
    """Attention of N independent query views per scene over a cached prefix of C views plus each view's own tile
    (csrc/attention_prefix.hip).  q / k / v: the query rows' thirds of the fused c_attn output, [B*N*L] rows; kp / vp: the cached
    K / V, [C*L] rows per scene, scenes ``prefix_stride`` elements apart.  ``bf16``: the tolerance arm (bf16 or fp32 tensors, one
    dtype for all five inputs; bf16 or fp32 ``out``); default: the fp32-equivalent arm (fp32 tensors).  ``ctx_len``: None (every view
    attends to all C cached views: the fixed-C entries, exactly as without the keyword) or an int32 device tensor [B*N], view (b, n)
    attending to the first ``ctx_len[b*N+n]`` cached views (0 <= length <= C, the caller's to ensure: the kernel clamps) and to itself
    (vf_attn_prefix_var_*).  A workgroup (4 / 2 consecutive views) costs what its longest member costs."""
    lib = _lib.load()
    if ctx_len is not None:
        _chk(ctx_len, torch.int32, 'ctx_len')
        if ctx_len.numel() != B * N or not ctx_len.is_contiguous():
            raise ValueError(f'attn_prefix: ctx_len int32 [B*N = {B * N}] contiguous expected, got {tuple(ctx_len.shape)}')
    if bf16:
        o16 = out.dtype == torch.bfloat16
        i16 = q.dtype == torch.bfloat16
        for t in (q, k, v, kp, vp):
            _chk(t, torch.bfloat16 if i16 else torch.float32, 'q/k/v/prefix')
        if ctx_len is not None:
            check(lib.vf_attn_prefix_var_bf16(_p(q), _p(k), _p(v), _p(kp), _p(vp), 1 if i16 else 0, _p(out if o16 else _f32(out)),
                                              1 if o16 else 0, B, H, C, N, L, dh, ldq, ldk, ldv, ldkp, ldvp, prefix_stride, ldo, _p(ctx_len),
                                              _stream()), 'vf_attn_prefix_var_bf16')
            return out
        check(lib.vf_attn_prefix_bf16(_p(q), _p(k), _p(v), _p(kp), _p(vp), 1 if i16 else 0, _p(out if o16 else _f32(out)), 1 if o16 else 0,
                                      B, H, C, N, L, dh, ldq, ldk, ldv, ldkp, ldvp, prefix_stride, ldo, _stream()), 'vf_attn_prefix_bf16')
        return out
    if ctx_len is not None:
        check(lib.vf_attn_prefix_var_f32eq(_p(_f32(q)), _p(_f32(k)), _p(_f32(v)), _p(_f32(kp)), _p(_f32(vp)), _p(_f32(out)), B, H, C, N, L, dh,
                                           ldq, ldk, ldv, ldkp, ldvp, prefix_stride, ldo, _p(ctx_len), _stream()), 'vf_attn_prefix_var_f32eq')
        return out
    check(lib.vf_attn_prefix_f32eq(_p(_f32(q)), _p(_f32(k)), _p(_f32(v)), _p(_f32(kp)), _p(_f32(vp)), _p(_f32(out)), B, H, C, N, L, dh,
                                   ldq, ldk, ldv, ldkp, ldvp, prefix_stride, ldo, _stream()), 'vf_attn_prefix_f32eq')
    return out


def attn_prefix_fork(q, k, v, kp, vp, kp2, vp2, out, B, H, C, C2, N, L, ldq, ldk, ldv, ldkp, ldvp, prefix_stride, ldkp2, ldvp2,
                     prefix_stride2, ldo, ctx_len, split, share, bf16=False, dh=64):
    """``attn_prefix(ctx_len=...)`` over a forked cache (vf_attn_prefix_fork_*): ``B`` CHILD scenes; child scene b reads the first
    ``split[b]`` views of parent scene ``b // share`` from kp / vp (``C`` views of room per parent scene, scenes ``prefix_stride``
    elements apart) and then its own views from kp2 / vp2 (``C2`` views of room per child scene, scenes ``prefix_stride2`` apart; with
    ``C2 = 0`` they may be None).  ``ctx_len`` int32 device [B*N] counts logical views, ``split`` int32 device [B].  A view gets the bits
    of ``attn_prefix(ctx_len=...)`` on the materialised cache (the parent's first split views, then the own views)."""
    lib = _lib.load()
    _chk(ctx_len, torch.int32, 'ctx_len')
    _chk(split, torch.int32, 'split')
    if ctx_len.numel() != B * N or not ctx_len.is_contiguous():
        raise ValueError(f'attn_prefix_fork: ctx_len int32 [B*N = {B * N}] contiguous expected, got {tuple(ctx_len.shape)}')
    if split.numel() != B or not split.is_contiguous():
        raise ValueError(f'attn_prefix_fork: split int32 [B = {B}] contiguous expected, got {tuple(split.shape)}')
    if (kp2 is None) != (vp2 is None) or (kp2 is None and C2 > 0):
        raise ValueError('attn_prefix_fork: kp2 and vp2 expected (None for both only with C2 = 0)')
    own = () if kp2 is None else (kp2, vp2)
    if bf16:
        o16 = out.dtype == torch.bfloat16
        i16 = q.dtype == torch.bfloat16
        for t in (q, k, v, kp, vp) + own:
            _chk(t, torch.bfloat16 if i16 else torch.float32, 'q/k/v/prefix')
        check(lib.vf_attn_prefix_fork_bf16(_p(q), _p(k), _p(v), _p(kp), _p(vp), 1 if i16 else 0, _p(out if o16 else _f32(out)),
                                           1 if o16 else 0, B, H, C, N, L, dh, ldq, ldk, ldv, ldkp, ldvp, prefix_stride, ldo, _p(ctx_len),
                                           _p(kp2), _p(vp2), C2, ldkp2, ldvp2, prefix_stride2, _p(split), share, _stream()),
              'vf_attn_prefix_fork_bf16')
        return out
    for t in (q, k, v, kp, vp, out) + own:
        _f32(t, 'q/k/v/prefix/out')
    check(lib.vf_attn_prefix_fork_f32eq(_p(q), _p(k), _p(v), _p(kp), _p(vp), _p(out), B, H, C, N, L, dh, ldq, ldk, ldv, ldkp, ldvp,
                                        prefix_stride, ldo, _p(ctx_len), _p(kp2), _p(vp2), C2, ldkp2, ldvp2, prefix_stride2, _p(split), share,
                                        _stream()), 'vf_attn_prefix_fork_f32eq')
    return out


def attn_prefix_bwd(q, k, v, kp, vp, dout, dqkv, B, H, C, N, L, ldq, ldk, ldv, ldkp, ldvp, prefix_stride, lddo, lddqkv, dh=64, ctx_len=None):
    """Backward of ``attn_prefix`` over the query views (csrc/attention_prefix_bwd.hip): q / k / v / kp / vp / ctx_len as there (bf16 or
    fp32 tensors, one dtype for all five; widened to fp32 on load, fp32 MFMA on either arm), ``dout`` fp32 [B*N*L][lddo] the gradient of
    the attention output -> ``dqkv`` fp32 [B*N*L][lddqkv] in the c_attn column order (V, Q, K): dV and dK of each view's own keys, dQ.
    The cache receives no gradient.  Every logical element of ``dqkv`` is written."""
    lib = _lib.load()
    if ctx_len is not None:
        _chk(ctx_len, torch.int32, 'ctx_len')
        if ctx_len.numel() != B * N or not ctx_len.is_contiguous():
            raise ValueError(f'attn_prefix_bwd: ctx_len int32 [B*N = {B * N}] contiguous expected, got {tuple(ctx_len.shape)}')
    i16 = q.dtype == torch.bfloat16
    for t in (q, k, v, kp, vp):
        _chk(t, torch.bfloat16 if i16 else torch.float32, 'q/k/v/prefix')
    check(lib.vf_attn_prefix_bwd_f32(_p(q), _p(k), _p(v), _p(kp), _p(vp), 1 if i16 else 0, _p(_f32(dout)), _p(_f32(dqkv)), B, H, C, N, L, dh,
                                     ldq, ldk, ldv, ldkp, ldvp, prefix_stride, lddo, lddqkv, _p(ctx_len), _stream()), 'vf_attn_prefix_bwd_f32')
    return dqkv


def kv_append(qkv, cache, B, K, L, d, ld_src, ld_dst, cache_stride, capacity, pos):
    """Append the keys and values of K new views per scene to a context cache with room (csrc/kv_append.hip): ``qkv`` = the new views'
    fused c_attn output, rows [B*K*L] of leading dimension ``ld_src``, thirds (V, Q, K); the V and K thirds of new view j of scene b go
    to the cache's view ``pos[b] + j`` (``cache``: ``capacity`` views of L rows per scene, leading dimension ``ld_dst``, scenes
    ``cache_stride`` elements apart), bit for bit, bf16 or fp32 (one dtype for both tensors).  ``pos``: int32 device tensor [B], each
    scene's own length.  One launch; nothing else of ``cache`` changes."""
    if qkv.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'kv_append: bf16 or fp32 tensors expected, got {qkv.dtype}')
    _chk(cache, qkv.dtype, 'cache')
    _chk(qkv, qkv.dtype, 'qkv')
    _chk(pos, torch.int32, 'pos')
    if pos.numel() != B or not pos.is_contiguous():
        raise ValueError(f'kv_append: pos int32 [B = {B}] contiguous expected, got {tuple(pos.shape)}')
    check(_lib.load().vf_kv_append(_p(qkv), _p(cache), qkv.element_size(), B, K, L, d, ld_src, ld_dst, cache_stride, capacity, _p(pos),
                                   _stream()), 'vf_kv_append')
    return cache


def kv_append_split(qkv, k, v, B, K, L, d, ld_src, ld_k, ld_v, k_stride, v_stride, capacity, pos):
    """``kv_append`` for a cache without a Q third (vf_kv_append_split): the K third of new view j of scene b goes to columns [0, d) of
    view ``pos[b] + j`` of ``k`` (``capacity`` views of L rows per scene, leading dimension ``ld_k``, scenes ``k_stride`` elements apart),
    the V third to the same rows of ``v`` (``ld_v``, ``v_stride``), bit for bit, bf16 or fp32 (one dtype for the three tensors).  One
    launch; nothing else of ``k`` and ``v`` changes."""
    if qkv.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'kv_append_split: bf16 or fp32 tensors expected, got {qkv.dtype}')
    _chk(k, qkv.dtype, 'k')
    _chk(v, qkv.dtype, 'v')
    _chk(qkv, qkv.dtype, 'qkv')
    _chk(pos, torch.int32, 'pos')
    if pos.numel() != B or not pos.is_contiguous():
        raise ValueError(f'kv_append_split: pos int32 [B = {B}] contiguous expected, got {tuple(pos.shape)}')
    check(_lib.load().vf_kv_append_split(_p(qkv), _p(k), _p(v), qkv.element_size(), B, K, L, d, ld_src, ld_k, ld_v, k_stride, v_stride,
                                         capacity, _p(pos), _stream()), 'vf_kv_append_split')
    return k, v


def kv_append_e4m3(qkv, kq, vq, kscale, vscale, B, K, H, L, ld_src, capacity, pos, q_view_stride=None, q_scene_stride=None,
                   s_view_stride=None, s_scene_stride=None):
    """The quantising ``kv_append`` (csrc/kv_append_e4m3.hip): the K and V thirds of new view j of scene b of ``qkv`` (fused c_attn rows
    [B*K*L] of leading dimension ``ld_src``, bf16 or fp32) go to slot ``pos[b] + j`` of the packed buffers — e4m3 tiles and scales as
    ``kv_pack_e4m3`` writes them for the same values, with its strides (default: tight [B*capacity, H, 64, 64] / [B*capacity, H]).
    ``pos``: int32 device tensor [B]; a slot outside [0, capacity) is skipped.  One launch; nothing else changes."""
    if qkv.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'kv_append_e4m3: bf16 or fp32 rows expected, got {qkv.dtype}')
    _chk(qkv, qkv.dtype, 'qkv')
    _chk(kq, torch.uint8, 'kq')
    _chk(vq, torch.uint8, 'vq')
    _chk(kscale, torch.float32, 'kscale')
    _chk(vscale, torch.float32, 'vscale')
    _chk(pos, torch.int32, 'pos')
    if pos.numel() != B or not pos.is_contiguous():
        raise ValueError(f'kv_append_e4m3: pos int32 [B = {B}] contiguous expected, got {tuple(pos.shape)}')
    qv, qs, sv, ss = _pack_strides(capacity, H, q_view_stride, q_scene_stride, s_view_stride, s_scene_stride)
    check(_lib.load().vf_kv_append_e4m3(_p(qkv), qkv.element_size(), _p(kq), _p(vq), _p(kscale), _p(vscale), B, K, H, L, ld_src, qv, qs, sv, ss,
                                        capacity, _p(pos), _stream()), 'vf_kv_append_e4m3')
    return kq, vq, kscale, vscale


def _pack_strides(C, H, q_view_stride, q_scene_stride, s_view_stride, s_scene_stride):
    """the tight packed layout [B*C, H, 64, 64] bytes / [B*C, H] scales where a stride is None"""
    qv = H * 4096 if q_view_stride is None else int(q_view_stride)
    sv = H if s_view_stride is None else int(s_view_stride)
    return (qv, C * qv if q_scene_stride is None else int(q_scene_stride), sv, C * sv if s_scene_stride is None else int(s_scene_stride))


def kv_pack_e4m3(cache, kq, vq, kscale, vscale, B, C, H, L, ld_src, cache_stride, lengths, q_view_stride=None, q_scene_stride=None,
                 s_view_stride=None, s_scene_stride=None):
    """Pack the K and V thirds of a context cache buffer to e4m3 tiles with one power-of-two scale per (scene, view, head)
    (csrc/kv_pack.hip): ``cache`` bf16 or fp32, ``C`` views of L rows per scene with leading dimension ``ld_src`` >= 3 * 64 H, thirds
    (V, Q, K), scenes ``cache_stride`` elements apart -> ``kq`` uint8 tiles [64 keys][64 features], ``vq`` uint8 tiles [64 features][64 keys]
    (tile (b, c, h) at byte b * q_scene_stride + c * q_view_stride + h * 4096; default: tight [B*C, H, 64, 64]) and ``kscale`` / ``vscale``
    fp32 (element b * s_scene_stride + c * s_view_stride + h; default: tight [B*C, H]).  ``lengths``: int32 device tensor [B]; views at or
    beyond a scene's length are neither read nor written.  One launch."""
    if cache.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'kv_pack_e4m3: a bf16 or fp32 cache expected, got {cache.dtype}')
    _chk(cache, cache.dtype, 'cache')
    _chk(kq, torch.uint8, 'kq')
    _chk(vq, torch.uint8, 'vq')
    _chk(kscale, torch.float32, 'kscale')
    _chk(vscale, torch.float32, 'vscale')
    _chk(lengths, torch.int32, 'lengths')
    if lengths.numel() != B or not lengths.is_contiguous():
        raise ValueError(f'kv_pack_e4m3: lengths int32 [B = {B}] contiguous expected, got {tuple(lengths.shape)}')
    qv, qs, sv, ss = _pack_strides(C, H, q_view_stride, q_scene_stride, s_view_stride, s_scene_stride)
    check(_lib.load().vf_kv_pack_e4m3(_p(cache), cache.element_size(), _p(kq), _p(vq), _p(kscale), _p(vscale), B, C, H, L, ld_src, cache_stride,
                                      qv, qs, sv, ss, _p(lengths), _stream()), 'vf_kv_pack_e4m3')
    return kq, vq, kscale, vscale


def attn_prefix_q8(q, k, v, kq, vq, kscale, vscale, out, B, H, C, N, L, ldq, ldk, ldv, ldo, ctx_len, q_view_stride=None, q_scene_stride=None,
                   s_view_stride=None, s_scene_stride=None, dh=64):
    """``attn_prefix(bf16=True, ctx_len=...)`` over a cache packed by ``kv_pack_e4m3`` (vf_attn_prefix_q8_bf16): ``kq`` / ``vq`` uint8
    tiles and ``kscale`` / ``vscale`` fp32 with the strides as there, ``C`` views of room per scene; q / k / v bf16 or fp32 (one dtype),
    ``out`` bf16 or fp32, ``ctx_len`` int32 device [B*N].  A view gets the bits of ``attn_prefix`` on the dequantised cache."""
    lib = _lib.load()
    _chk(ctx_len, torch.int32, 'ctx_len')
    if ctx_len.numel() != B * N or not ctx_len.is_contiguous():
        raise ValueError(f'attn_prefix_q8: ctx_len int32 [B*N = {B * N}] contiguous expected, got {tuple(ctx_len.shape)}')
    o16 = out.dtype == torch.bfloat16
    i16 = q.dtype == torch.bfloat16
    for t in (q, k, v):
        _chk(t, torch.bfloat16 if i16 else torch.float32, 'q/k/v')
    _chk(kq, torch.uint8, 'kq')
    _chk(vq, torch.uint8, 'vq')
    _chk(kscale, torch.float32, 'kscale')
    _chk(vscale, torch.float32, 'vscale')
    qv, qs, sv, ss = _pack_strides(C, H, q_view_stride, q_scene_stride, s_view_stride, s_scene_stride)
    check(lib.vf_attn_prefix_q8_bf16(_p(q), _p(k), _p(v), _p(kq), _p(vq), _p(kscale), _p(vscale), 1 if i16 else 0, _p(out if o16 else _f32(out)),
                                     1 if o16 else 0, B, H, C, N, L, dh, ldq, ldk, ldv, qv, qs, sv, ss, ldo, _p(ctx_len), _stream()),
          'vf_attn_prefix_q8_bf16')
    return out


def attn_spatial_supported(HW, C):
    return (HW, C) in ((256, 256), (64, 512), (64, 256))


def attn_spatial(qkv, n_img, HW, C, scale, out=None, x3h=False):
    """fused single-head attention of the VQGAN AttnBlock: qkv [n_img*HW][3C] (q|k|v) -> [n_img*HW][C]; scores stay on chip.
    ``x3h``: the fp32-equivalent three-product fp16 form (vf_attn_spatial_x3h) instead of the native f32 MFMA"""
    if out is None:
        out = torch.empty((n_img * HW, C), dtype=torch.float32, device=qkv.device)
    fn = _lib.load().vf_attn_spatial_x3h if x3h else _lib.load().vf_attn_spatial_f32
    check(fn(_p(_f32(qkv)), _p(_f32(out)), n_img, HW, C, qkv.stride(0), out.stride(0), scale, _stream()),
          'vf_attn_spatial_x3h' if x3h else 'vf_attn_spatial_f32')
    return out


def softmax_rows_(x, rows, n, scale=1.0):
    check(_lib.load().vf_softmax_rows_f32(_p(_f32(x)), rows, n, scale, _stream()), 'vf_softmax_rows_f32')
    return x


def layernorm(x, gamma, beta, rows, d, eps=1e-5, out=None, out_bf16=False):
    """``out_bf16``: write the normalised rows as bf16 (for a bf16-GEMM consumer: ``igemm(..., bf16=True, a16=True)``)"""
    if out_bf16:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if out is None else _chk(out, torch.bfloat16, 'out')
        check(_lib.load().vf_layernorm_bf16out_f32(_p(_f32(x)), _p(_f32(gamma)), _p(_f32(beta)), _p(out), rows, d, eps, _stream()),
              'vf_layernorm_bf16out_f32')
        return out
    if out is None:
        out = torch.empty_like(x)
    check(_lib.load().vf_layernorm_f32(_p(_f32(x)), _p(_f32(gamma)), _p(_f32(beta)), _p(out), rows, d, eps, _stream()),
          'vf_layernorm_f32')
    return out


def embed_sum(ids_i32, wte, wpe, add, BS, L, d, vocab):
    out = torch.empty((BS * L, d), dtype=torch.float32, device=wte.device)
    check(_lib.load().vf_embed_sum_f32(_p(_chk(ids_i32, torch.int32, 'ids')), _p(_f32(wte)), _p(_f32(wpe)),
                                       _p(_f32(add)), _p(out), BS, L, d, vocab, _stream()), 'vf_embed_sum_f32')
    return out


def dense_small_k(x, W, b, rows, K, N, gelu):
    out = torch.empty((rows, N), dtype=torch.float32, device=x.device)
    check(_lib.load().vf_dense_small_k_gelu_f32(_p(_f32(x)), _p(_f32(W)), _p(b), _p(out), rows, K, N,
                                                1 if gelu else 0, _stream()), 'vf_dense_small_k_gelu_f32')
    return out


def argmax_rows(x, rows, n, ld=None):
    idx = torch.empty(rows, dtype=torch.int64, device=x.device)
    check(_lib.load().vf_argmax_rows_f32(_p(_f32(x)), rows, n, n if ld is None else ld, _p(idx), _stream()),
          'vf_argmax_rows_f32')
    return idx


def lmhead_argmax_supported(K, N):
    return K in (128, 768) and N % 128 == 0


def lmhead_argmax_bf16(h, w_packed_bf16, M, K, N, want_max=False):
    """fused tied LM head + arg-max (bf16 arm): h [M][K] fp32 or bf16 rows, w_packed_bf16 = pack_dense_nk_bf16(wte, n_rows=N).
    Returns idx int64 [M] (and the winning logits if ``want_max``); the [M][N] logits are never materialised."""
    idx = torch.empty(M, dtype=torch.int64, device=h.device)
    mx = torch.empty(M, dtype=torch.float32, device=h.device) if want_max else None
    h16 = h.dtype == torch.bfloat16
    _chk(h, torch.bfloat16 if h16 else torch.float32, 'h')
    check(_lib.load().vf_lmhead_argmax_bf16(_p(h), 1 if h16 else 0, h.stride(0), _p(_chk(w_packed_bf16, torch.bfloat16, 'w_packed')), M, K, N,
                                            _p(idx), _p(mx) if mx is not None else None, _stream()), 'vf_lmhead_argmax_bf16')
    return (idx, mx) if want_max else idx


SCORE_OUTPUTS = ('idx', 'max_logit', 'lse', 'target_logit', 'entropy')


def _score_want(want, target):
    want = tuple(want)
    if not want or any(w not in SCORE_OUTPUTS for w in want):
        raise ValueError(f'want: a non-empty subset of {SCORE_OUTPUTS} expected, got {want}')
    if 'target_logit' in want and target is None:
        raise ValueError("want 'target_logit': target expected")
    return want


def _score_outputs(want, rows, dev, target):
    if target is not None:
        _chk(target, torch.int32, 'target')
        if target.numel() != rows or not target.is_contiguous():
            raise ValueError(f'target: {rows} contiguous int32 expected, got {tuple(target.shape)}')
    return {w: torch.empty(rows, dtype=torch.int64 if w == 'idx' else torch.float32, device=dev) for w in want}


def lmhead_score_supported(K, N):
    return K in (128, 768) and N % 128 == 0


def lmhead_score_bf16(h, w_packed_bf16, M, K, N, target=None, want=SCORE_OUTPUTS):
    """fused tied LM head + soft-max statistics (bf16 arm): h [M][K] fp32 or bf16 rows, w_packed_bf16 = pack_dense_nk_bf16(wte, n_rows=N),
    target int32 [M] or None.  Returns a dict of the outputs named in ``want`` (SCORE_OUTPUTS; idx int64, the rest fp32, [M] each); the
    [M][N] logits are never materialised."""
    want = _score_want(want, target)
    h16 = h.dtype == torch.bfloat16
    _chk(h, torch.bfloat16 if h16 else torch.float32, 'h')
    out = _score_outputs(want, M, h.device, target)
    check(_lib.load().vf_lmhead_score_bf16(_p(h), 1 if h16 else 0, h.stride(0), _p(_chk(w_packed_bf16, torch.bfloat16, 'w_packed')), M, K, N,
                                           _p(target), *(_p(out.get(w)) for w in SCORE_OUTPUTS), _stream()), 'vf_lmhead_score_bf16')
    return out


def logits_score(logits, rows, N, target=None, want=SCORE_OUTPUTS, ld=None):
    """the same statistics from materialised fp32 logits [rows][ld >= N] (the fp32-equivalent arms; shapes the fused kernel refuses)"""
    want = _score_want(want, target)
    _f32(logits, 'logits')
    out = _score_outputs(want, rows, logits.device, target)
    check(_lib.load().vf_logits_score_f32(_p(logits), rows, N, N if ld is None else ld, _p(target), *(_p(out.get(w)) for w in SCORE_OUTPUTS),
                                          _stream()), 'vf_logits_score_f32')
    return out


def score_views(stats, target, views, L):
    """per-view summary of lmhead_score_bf16 / logits_score results (all five outputs) for ``views`` views of L rows: (token_log_prob
    [views*L], confidence [views*L], log_likelihood [views] summed in token order, accuracy [views]), fp32"""
    dev = target.device
    tlp, conf = (torch.empty(views * L, dtype=torch.float32, device=dev) for _ in range(2))
    ll, acc = (torch.empty(views, dtype=torch.float32, device=dev) for _ in range(2))
    check(_lib.load().vf_score_views_f32(_p(_f32(stats['target_logit'])), _p(_f32(stats['lse'])), _p(_f32(stats['max_logit'])),
                                         _p(_chk(stats['idx'], torch.int64, 'idx')), _p(_chk(target, torch.int32, 'target')), views, L,
                                         _p(tlp), _p(conf), _p(ll), _p(acc), _stream()), 'vf_score_views_f32')
    return tlp, conf, ll, acc


def match_views(logits, lse, idx, codes, B, M, P, L, V, ld=None, want_accuracy=True):
    """P photos against M cameras per scene from the M scored views (vf_match_views_f32; include/vf_hip.h has the definition): ``logits``
    fp32 [B*M*L][ld >= V], ``lse`` fp32 and ``idx`` int64 [B*M*L] as ``logits_score`` gives them (``idx`` may be None without
    ``want_accuracy``), ``codes`` int32 [B or 1, P, L] (a leading 1: one photo set shared by all scenes).  Returns (log_likelihood,
    accuracy or None), fp32 [B, M, P] each: camera-major, the sum of a photo's token log-probabilities as one fp32 chain in token order
    and the share of its tokens the view predicts."""
    _f32(logits, 'logits')
    _f32(lse, 'lse')
    _chk(codes, torch.int32, 'codes')
    ld = V if ld is None else ld
    if want_accuracy and idx is None:
        raise ValueError('match_views: accuracy needs idx')
    if idx is not None:
        _chk(idx, torch.int64, 'idx')
    if codes.dim() != 3 or codes.shape[0] not in (1, B) or tuple(codes.shape[1:]) != (P, L):
        raise ValueError(f'codes: int32 [{B} or 1, {P}, {L}] expected, got {tuple(codes.shape)}')
    # the scene stride is the leading dimension's; a photo's L codes and a scene's P photos lie densely
    stride = codes.stride(0) if codes.shape[0] > 1 else 0
    if P and (codes.stride(2) != 1 or (P > 1 and codes.stride(1) != L) or (stride and stride < P * L)):
        raise ValueError(f'codes: dense photos [{P}, {L}] per scene and a scene stride >= {P * L} expected, got strides {codes.stride()}')
    if (lse.numel() != B * M * L or not lse.is_contiguous() or (idx is not None and (idx.numel() != B * M * L or not idx.is_contiguous()))
            or ld < V):
        raise ValueError(f'match_views: contiguous lse and idx [{B * M * L}] and ld >= {V} expected, got {tuple(lse.shape)}, '
                         f'{None if idx is None else tuple(idx.shape)}, ld {ld}')
    ll = torch.empty((B, M, P), dtype=torch.float32, device=logits.device)
    acc = torch.empty((B, M, P), dtype=torch.float32, device=logits.device) if want_accuracy else None
    check(_lib.load().vf_match_views_f32(_p(logits), ld, _p(lse), _p(idx) if want_accuracy else None, _p(codes), stride, B, M, P, L, V, _p(ll),
                                         _p(acc), _stream()), 'vf_match_views_f32')
    return ll, acc


SAMPLE_OUTPUTS = ('idx', 'logp', 'kept', 'thr')


def sample_rows(logits, rows, N, temperature=1.0, top_k=0, top_p=1.0, seed=0, row_id=None, n_samples=1, ld=None, want=('idx', 'logp')):
    """``n_samples`` reproducible draws per row of fp32 logits [rows][ld >= N] under temperature, top-k and top-p (vf_sample_rows_f32;
    include/vf_hip.h has the definitions).  ``row_id`` int64 [rows] or None (the row's number) keys the noise together with ``seed`` and
    the sample index.  Returns a dict of the outputs named in ``want`` (SAMPLE_OUTPUTS): idx int64 [rows, S], logp fp32 [rows, S] (log
    probability of each draw under the filtered distribution), kept int32 [rows] (size of the set drawn from), thr fp32 [rows] (the
    smallest kept logit / temperature)."""
    want = tuple(want)
    if not want or any(w not in SAMPLE_OUTPUTS for w in want):
        raise ValueError(f'want: a non-empty subset of {SAMPLE_OUTPUTS} expected, got {want}')
    _f32(logits, 'logits')
    S = int(n_samples)
    ldv = N if ld is None else int(ld)
    if rows < 0 or N < 1 or ldv < N or not logits.is_contiguous() or logits.numel() < (rows - 1) * ldv + N * (rows > 0):
        raise ValueError(f'logits: {rows} contiguous rows of {N} with ld {ldv} expected, got {tuple(logits.shape)}')
    if row_id is not None:
        _chk(row_id, torch.int64, 'row_id')
        if row_id.numel() != rows or not row_id.is_contiguous():
            raise ValueError(f'row_id: {rows} contiguous int64 expected, got {tuple(row_id.shape)}')
    dev = logits.device
    shapes = dict(idx=((rows, max(S, 0)), torch.int64), logp=((rows, max(S, 0)), torch.float32), kept=((rows,), torch.int32),
                  thr=((rows,), torch.float32))
    out = {w: torch.empty(shapes[w][0], dtype=shapes[w][1], device=dev) for w in SAMPLE_OUTPUTS if w == 'idx' or w in want}
    check(_lib.load().vf_sample_rows_f32(_p(logits), rows, N, N if ld is None else ld, float(temperature), int(top_k), float(top_p),
                                         int(seed) & 0xFFFFFFFF, _p(row_id), S, *(_p(out.get(w)) for w in SAMPLE_OUTPUTS), _stream()),
          'vf_sample_rows_f32')
    return {w: out[w] for w in want}


def sample_views(logp, views, L, n_samples):
    """log-likelihood of sampled views: ``logp`` fp32 [views * L, S] (sample_rows') -> fp32 [views, S], each the sum over the view's L
    tokens as one fp32 chain in token order"""
    _f32(logp, 'logp')
    S = int(n_samples)
    if logp.numel() != views * L * S or not logp.is_contiguous():
        raise ValueError(f'logp: contiguous [{views * L}, {S}] expected, got {tuple(logp.shape)}')
    ll = torch.empty((views, S), dtype=torch.float32, device=logp.device)
    check(_lib.load().vf_sample_views_f32(_p(logp), views, L, S, _p(ll), _stream()), 'vf_sample_views_f32')
    return ll


MIX_OUTPUTS = ('out', 'kept', 'thr')
MIX_ROWS_PER_GROUP = 16          # rows that share one workgroup's codebook tiles (csrc/mix_rows.hip); no result depends on it


def mix_rows_supported(D, N):
    """the shapes vf_mix_rows_f32 takes: the row in registers and D in whole pairs of 16-feature MFMA tiles"""
    return 1 <= int(N) <= 1024 and 1 <= int(D) <= 256 and int(D) % 32 == 0


def mix_rows(logits, rows, N, E, D, temperature=1.0, top_k=0, top_p=1.0, ld=None, ldE=None, want=('out',)):
    """The mean of the distribution ``sample_rows`` draws from, in the codebook's latent space (vf_mix_rows_f32; include/vf_hip.h has the
    definitions): fp32 logits [rows][ld >= N] and the codebook ``E`` fp32 [D][ldE >= N] (``codebook_gather``'s layout) -> a dict of the
    outputs named in ``want`` (MIX_OUTPUTS): out fp32 [rows, D] = sum over the kept codes of p_n E[:, n], kept int32 [rows] and thr fp32
    [rows] (``sample_rows``' bits).  ``top_k = 1`` is ``codebook_gather`` of the arg-max."""
    want = tuple(want)
    if not want or any(w not in MIX_OUTPUTS for w in want):
        raise ValueError(f'want: a non-empty subset of {MIX_OUTPUTS} expected, got {want}')
    _f32(logits, 'logits')
    _f32(E, 'E')
    ldv, ldEv = N if ld is None else int(ld), N if ldE is None else int(ldE)
    if rows < 0 or N < 1 or ldv < N or not logits.is_contiguous() or logits.numel() < (rows - 1) * ldv + N * (rows > 0):
        raise ValueError(f'logits: {rows} contiguous rows of {N} with ld {ldv} expected, got {tuple(logits.shape)}')
    if D < 1 or ldEv < N or not E.is_contiguous() or E.numel() < (D - 1) * ldEv + N:
        raise ValueError(f'E: {D} contiguous rows of {N} with ldE {ldEv} expected, got {tuple(E.shape)}')
    dev = logits.device
    shapes = dict(out=((rows, D), torch.float32), kept=((rows,), torch.int32), thr=((rows,), torch.float32))
    out = {w: torch.empty(shapes[w][0], dtype=shapes[w][1], device=dev) for w in MIX_OUTPUTS if w == 'out' or w in want}
    if rows == 0:                                                    # (an empty batch owns no memory: its pointers are null)
        return {w: out[w] for w in want}
    check(_lib.load().vf_mix_rows_f32(_p(logits), rows, N, ldv, float(temperature), int(top_k), float(top_p), _p(E), D, ldEv,
                                      _p(out['out']), D, _p(out.get('kept')), _p(out.get('thr')), _stream()), 'vf_mix_rows_f32')
    return {w: out[w] for w in want}


def postprocess_u8(x):
    x = _f32(x).contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(_lib.load().vf_postprocess_u8(_p(x), _p(out), x.numel(), _stream()), 'vf_postprocess_u8')
    return out


def resize_u8(images, image_size, method=None):
    """``resize`` of viewformer/data/_common.py:47-61 on NHWC uint8 images [n,H,W,C]: identity when H == image_size, otherwise torch
    'nearest' when enlarging / bilinear (align_corners=False) when shrinking unless ``method`` says otherwise; uint8 out"""
    if method not in (None, 'nearest', 'bilinear'):
        raise ValueError("method must be None, 'nearest' or 'bilinear'")
    n, H, W, C = images.shape
    # resize() tests the NHWC batch's shape[-2] (= W), then resize_th() tests the NCHW tensor's shape[-2] (= H): either match
    # returns the frames untouched (data/_common.py:26-27,54-55); the enlarge/shrink choice below uses H (:34-37)
    if W == image_size or H == image_size:
        return images
    if method is None:
        method = 'nearest' if image_size > H else 'bilinear'
    src = _chk(images.contiguous(), torch.uint8, 'images')
    out = torch.empty((n, image_size, image_size, C), dtype=torch.uint8, device=images.device)
    check(_lib.load().vf_resize_u8(_p(src), _p(out), n, H, W, image_size, image_size, C, 1 if method == 'bilinear' else 0, _stream()),
          'vf_resize_u8')
    return out


def image_metrics_u8(a, b):
    """Per pair of NHWC uint8 images [n,H,W,C] on the GPU (vf_image_metrics_u8): -> (sums int64 [n,2] = {sum (a-b)^2, sum |a-b|}, exact;
    ssim float64 [n] = mean of the reference's per-pixel SSIM, viewformer/utils/metrics.py:17-69 with K1 = 1 as SSIMMetric calls it, :183).
    H, W >= 7, C <= 4.  One launch pair, no synchronisation; the values of an image do not depend on the rest of the batch."""
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError(f'image_metrics_u8: two [n,H,W,C] batches of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}')
    a = _chk(a, torch.uint8, 'a').contiguous()
    b = _chk(b, torch.uint8, 'b').contiguous()
    n, H, W, C = a.shape
    if n == 0:
        return torch.empty((0, 2), dtype=torch.int64, device=a.device), torch.empty(0, dtype=torch.float64, device=a.device)
    lib = _lib.load()
    ws =torch.empty(max(int(lib.vf_image_metrics_workspace_bytes(n, H, W, C)), 8), dtype=torch.uint8, device=a.device)
    sums = torch.empty((n, 2), dtype=torch.int64, device=a.device)
    ssim = torch.empty(n, dtype=torch.float64, device=a.device)
    check(lib.vf_image_metrics_u8(_p(a), _p(b), n, H, W, C, _p(sums), _p(ssim), _p(ws), _stream()), 'vf_image_metrics_u8')
    return sums, ssim


def camera_knn(db, queries, k, pos_weight=0.3, return_dist=False):
    """For each query camera [Q,7] the ``k`` cameras of ``db`` [N,7] (fp32, on the GPU) nearest in the pose distance of
    viewformer/evaluate/evaluate_sevenscenes.py:36-45 (vf_camera_knn_f32): idx int32 [Q,k] ascending, ties to the lowest index; with
    ``return_dist`` also the distances fp32 [Q,k].  1 <= k <= 32, k <= N.  One or two launches on the current stream, no synchronisation;
    a query's row does not depend on the other queries of the call."""
    if db.dim() != 2 or db.shape[1] != 7 or queries.dim() != 2 or queries.shape[1] != 7:
        raise ValueError(f'camera_knn: db [N,7] and queries [Q,7] expected, got {tuple(db.shape)} and {tuple(queries.shape)}')
    db = _f32(db, 'db').contiguous()
    queries = _f32(queries, 'queries').contiguous()
    N, Q, k = db.shape[0], queries.shape[0], int(k)
    idx = torch.empty((Q, k), dtype=torch.int32, device=db.device)
    dist = torch.empty((Q, k), dtype=torch.float32, device=db.device) if return_dist else None
    lib = _lib.load()
    ws = torch.empty(max(int(lib.vf_camera_knn_workspace_bytes(N, Q, k)), 8), dtype=torch.uint8, device=db.device)
    check(lib.vf_camera_knn_f32(_p(db), N, _p(queries), Q, k, float(pos_weight), _p(idx), _p(dist), _p(ws), _stream()), 'vf_camera_knn_f32')
    return (idx, dist) if return_dist else idx


def codebook_distances(E, D, K):
    """The distance table of a codebook (vf_codebook_dist_table_f32): ``E`` feature-major [D][ld >= K] fp32 on the GPU, as ``VQGAN._E``
    holds it -> fp32 [K,K], T[a][b] = ||e_a - e_b||^2 summed over the features in order: exactly symmetric, exactly 0 on the diagonal.
    One launch on the current stream, no synchronisation."""
    D, K = int(D), int(K)
    if not isinstance(E, torch.Tensor) or E.dim() != 2 or not E.is_cuda or E.dtype != torch.float32:
        raise ValueError('codebook_distances: a 2-D fp32 codebook [D][K] on the GPU expected')
    if E.shape[0] != D or E.shape[1] < K or K < 1 or D < 1 or E.stride(1) != 1 or (D > 1 and E.stride(0) < K):
        raise ValueError(f'codebook_distances: E [D = {D}][>= K = {K}] with unit column stride expected, got {tuple(E.shape)} '
                         f'(strides {tuple(E.stride())})')
    table = torch.empty((K, K), dtype=torch.float32, device=E.device)
    check(_lib.load().vf_codebook_dist_table_f32(_p(E), D, K, E.stride(0) if D > 1 else max(E.stride(0), K), _p(table), _stream()),
          'vf_codebook_dist_table_f32')
    return table


def _code_rows(x, name):
    """int32 code maps [n,t,t] or [n,t*t] on the GPU (rows may be strided) -> (the tensor, n, t*t, row stride)"""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.dtype != torch.int32:
        raise ValueError(f'code_knn: {name} must be an int32 tensor [n,t,t] or [n,t*t]')
    if x.dim() == 3:
        if x.shape[1] != x.shape[2]:
            raise ValueError(f'code_knn: {name} {tuple(x.shape)} is not a batch of square code maps')
        x = x.reshape(x.shape[0], -1)
    if x.shape[1] < 1:
        raise ValueError(f'code_knn: {name} {tuple(x.shape)} holds no codes')
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, x.shape[0], x.shape[1], (x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1]))


def code_knn(db_codes, query_codes, table, k, window=0, exclude=None, return_dist=False):
    """For each query code map the ``k`` maps of ``db_codes`` nearest in the windowed one-sided Chamfer distance over ``table``
    (``codebook_distances``; vf_code_knn_f32): sum over the grid positions p of the smallest table[q[p]][m[p']] over the positions p'
    within ``window`` tokens of p.  ``window=0``: the squared L2 distance of the two quantised latent maps.  ``db_codes`` int32 [N,t,t]
    or [N,t*t], ``query_codes`` likewise [Q,...] (on the GPU), ``exclude``: None or one database row per query (int [Q], -1: none) that
    the query must not return (a leave-one-out search of a bank against itself).  -> idx int32 [Q,k] ascending, ties to the lowest index;
    with ``return_dist`` also the distances fp32 [Q,k].  1 <= k <= 32, k <= N (N - 1 with ``exclude``), t <= 16, 0 <= window <= t - 1.
    One or two launches on the current stream, no synchronisation; a query's row does not depend on the other queries of the call."""
    db, N, P, ld_db = _code_rows(db_codes, 'db_codes')
    qs, Q, Pq, ld_q = _code_rows(query_codes, 'query_codes')
    t = int(round(P ** 0.5))
    if t * t != P or Pq != P:
        raise ValueError(f'code_knn: {P} and {Pq} codes per row: one square grid expected')
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[0] != table.shape[1] or table.dtype != torch.float32:
        raise ValueError('code_knn: table must be a square fp32 tensor [K,K]')
    if not (db.is_cuda and qs.is_cuda and table.is_cuda) or not db.device == qs.device == table.device:
        raise ValueError('code_knn: db_codes, query_codes and table must live on one GPU (no CPU fallback for the hot path)')
    table = table.contiguous()
    k, window = int(k), int(window)
    if exclude is not None:
        exclude = torch.as_tensor(exclude)
        if exclude.numel() != Q or exclude.is_floating_point():
            raise ValueError(f'code_knn: exclude must hold one database row per query ({Q}), got {tuple(exclude.shape)} {exclude.dtype}')
        exclude = exclude.reshape(Q).to(device=db.device, dtype=torch.int32).contiguous()
    if not 1 <= k <= min(32, N - (exclude is not None)) or not 0 <= window <= t - 1 or t > 16 or not 1 <= table.shape[0] <= 4096:
        raise ValueError(f'code_knn: k = {k} (at most 32) of N = {N} rows{" less the excluded one" if exclude is not None else ""}, '
                         f'window = {window} on a {t} x {t} grid (at most 16 x 16), {table.shape[0]} codes (at most 4096)')
    idx = torch.empty((Q, k), dtype=torch.int32, device=db.device)
    dist = torch.empty((Q, k), dtype=torch.float32, device=db.device) if return_dist else None
    lib = _lib.load()
    ws = torch.empty(max(int(lib.vf_code_knn_workspace_bytes(N, Q, k)), 8), dtype=torch.uint8, device=db.device)
    check(lib.vf_code_knn_f32(_p(db), N, ld_db, _p(qs), Q, ld_q, t, _p(table), table.shape[0], window, _p(exclude), k, _p(idx), _p(dist),
                              _p(ws), _stream()), 'vf_code_knn_f32')
    return (idx, dist) if return_dist else idx


def pose_tail_supported(K, L):
    """shapes vf_pose_tail_f32 takes: K features per row (a multiple of 4, at most 2048), L tokens per view (at most 256)"""
    return K % 4 == 0 and 4 <= K <= 2048 and 1 <= L <= 256


def pose_tail(x, W, b, position_multiplier, views, L, want_raw=False, want_tokens=False):
    """The localization head's tail in one launch (vf_pose_tail_f32): x [views*L, K] fp32 rows (row stride a multiple of 4; the GELU
    output of pose_classifier.c_fc), W [K,7] as stored, b [7] or None -> (cameras [views,7], tokens [views,L,7] | None,
    raw [views,L,7] | None): raw = x @ W + b, tokens = geometry.pose_head_postprocess(raw, position_multiplier), cameras =
    geometry.reduce_cameras(tokens, -2).  A view's outputs do not depend on the other views of the call or on the optional outputs."""
    if x.dim() != 2 or x.shape[0] != views * L or x.stride(1) != 1 or W.dim() != 2 or tuple(W.shape) != (x.shape[1], 7):
        raise ValueError(f'pose_tail: x [views*L = {views * L}, K] with unit column stride and W [K,7] expected, got {tuple(x.shape)} '
                         f'(strides {tuple(x.stride())}) and {tuple(W.shape)}')
    if b is not None and b.numel() != 7:
        raise ValueError(f'pose_tail: b [7] expected, got {tuple(b.shape)}')
    K = x.shape[1]
    W = _f32(W, 'W').contiguous()
    b = _f32(b, 'b').contiguous() if b is not None else None
    dev = x.device
    cameras = torch.empty((views, 7), dtype=torch.float32, device=dev)
    tokens = torch.empty((views, L, 7), dtype=torch.float32, device=dev) if want_tokens else None
    raw = torch.empty((views, L, 7), dtype=torch.float32, device=dev) if want_raw else None
    check(_lib.load().vf_pose_tail_f32(_p(_f32(x, 'x')), x.stride(0) if views * L > 1 else max(x.stride(0), K), _p(W), _p(b),
                                       float(position_multiplier), views, L, K, _p(raw), _p(tokens), _p(cameras), _stream()), 'vf_pose_tail_f32')
    return cameras, tokens, raw
