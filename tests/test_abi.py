"""CPU: the C-ABI shared library loads and exports every symbol include/vf_hip.h declares;
host-only queries and argument validation work without a GPU (no compute calls here)."""
import ctypes
import os
import re

import pytest

from conftest import REPO


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _declared():
    src = open(os.path.join(REPO, 'include', 'vf_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(vf_[a-z0-9_]+)\s*\(', src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from viewformer_amd import _lib
    declared = _declared()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in vf_hip.h but not exported'
    assert sorted(_lib.EXPORTS) == declared, set(_lib.EXPORTS) ^ set(declared)


def test_host_queries(lib):
    assert lib.vf_abi_version() == 20
    # the struct mirrors of the binding have the library's layout (checked again at load time: a mismatch raises)
    import ctypes
    from viewformer_amd import _lib as L
    assert int(lib.vf_sizeof_igemm_args()) == ctypes.sizeof(L.VfIgemmArgs)
    assert int(lib.vf_sizeof_pack_desc()) == L.PACK_DESC_BYTES
    assert int(lib.vf_sizeof_adamw_pack_desc()) == L.ADAMW_PACK_DESC_BYTES
    assert lib.vf_build_arch() == b'gfx950'
    # [chunks=4][taps=9][nblk=1][32][128]
    assert lib.vf_igemm_packed_floats(128, 128, 9) == 4 * 9 * 32 * 128
    assert lib.vf_igemm_packed_floats(768, 3, 1) == 24 * 32 * 32          # N=3 padded to the 32-wide tile
    assert lib.vf_igemm_packed_floats(0, 3, 1) == 0
    assert lib.vf_vq_packed_floats(256, 1024) == 256 * 1024
    assert lib.vf_vq_packed_floats(32, 64) == 32 * 128                     # codes padded to 128
    assert lib.vf_groupnorm_workspace_bytes(4, 16384, 128) == 4 * 64 * 256 * 2 * 4


def test_adamw_pack_table_validation_is_host_side(lib):
    """vf_adamw_pack_check (round 6) validates a HOST copy of the fused optimizer's descriptor table — no device, no launch: sorted disjoint ranges
    inside the flat buffer, whole 128-blocks both ways, 16-byte aligned destinations, at least one destination, at most 256 descriptors."""
    import numpy as np
    from viewformer_amd import _lib as L
    dt = np.dtype([('offset', '<i8'), ('dst_kn', '<u8'), ('dst_nk', '<u8'), ('rows', '<i4'), ('cols', '<i4'), ('nodecay', '<i4'), ('reserved', '<i4')])
    assert dt.itemsize == L.ADAMW_PACK_DESC_BYTES

    def check(rows, n=1 << 24):
        a = np.array(rows, dtype=dt)
        return lib.vf_adamw_pack_check(a.ctypes.data, len(a), n)
    ok = [(0, 4096, 8192, 128, 256, 0, 0), (128 * 256, 0, 16384, 256, 128, 1, 0)]
    assert check(ok) == 0
    assert check(ok[::-1]) == -1                                           # not sorted
    assert check([ok[0], (100, 4096, 0, 128, 128, 0, 0)]) == -1            # overlapping
    assert check([(0, 0, 0, 128, 128, 0, 0)]) == -1                        # no destination
    assert check([(0, 4096, 0, 128, 128, 0, 0)], n=128 * 128 - 4) == -1    # past the end of the flat buffer
    assert check([(0, 4096, 0, 64, 128, 0, 0)]) == -2                      # rows % 128
    assert check([(0, 4096, 0, 128, 192, 0, 0)]) == -2                     # cols % 128
    assert check([(2, 4096, 0, 128, 128, 0, 0)]) == -2                     # offset % 4
    assert check([(0, 4100, 0, 128, 128, 0, 0)]) == -2                     # destination alignment
    assert check([(i * 128 * 128, 4096, 0, 128, 128, 0, 0) for i in range(257)], n=1 << 30) == -2
    assert lib.vf_adamw_pack_check(None, 1, 16) == -1


def test_shipped_library_has_no_developer_switch_compiled_in(lib):
    """The kernel sources hold no compile-time knobs: the one developer switch left, -DVF_X_TRINTRIN (the compiler-ordered reference
    build of the DMA-ring kernels that tests/test_hip_ring_stress.py compares with), registers its name when a translation unit is built
    with it (csrc/vf_common.h).  The product library must register none, and every macro that a preprocessor conditional in csrc/ tests
    must be such a registered switch, so that no unregistered knob with a default can select a path no build or test exercises."""
    names = [lib.vf_build_flag_name(i) for i in range(lib.vf_build_flags())]
    assert lib.vf_build_flags() == 0, f'libvf_hip.so was built with developer switches: {names}'
    assert lib.vf_build_flag_name(0) is None
    csrc = os.path.join(REPO, 'viewformer_amd', 'csrc')
    known = set(re.findall(r'^VF_REG_FLAG\((\w+)\)', open(os.path.join(csrc, 'vf_common.h')).read(), flags=re.M))
    used = {}
    for f in sorted(os.listdir(csrc)):
        if f.endswith(('.hip', '.h')):
            src = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(csrc, f)).read(), flags=re.S).replace('\\\n', ' ')
            for cond in re.findall(r'^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$', src, flags=re.M):
                for name in re.findall(r'\b[A-Za-z_]\w*\b', cond.split('//')[0]):
                    if name != 'defined':
                        used.setdefault(name, f)
    assert {n: f for n, f in used.items() if n not in known} == {}


def test_library_reads_no_environment_and_its_switches_are_explicit(lib):
    """No run-time knob can change a result behind the caller's back: libvf_hip.so does not import getenv / secure_getenv at all (round 3
    shipped several per-launch getenv calls, one of which selected a kernel with wrong results); the only run-time switches are
    vf_select's — each between two kernels the GPU tests assert bit-identical, except VF_SEL_CONV_X3H_K32 (two MFMA shapes of the x3h
    convolution: held to the same fp32-equivalence bound and the same 20 480 reference tokens) and VF_SEL_ATTN_DMA (the LDS-DMA attention
    re-rounds a pre-scaled q: within 1e-2 of the register-staged kernel, both inside the bf16 arm's tolerance) — and they validate their
    arguments."""
    import subprocess
    from viewformer_amd import _lib
    syms = subprocess.run(['nm', '-D', '--undefined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert 'getenv' not in syms, [l for l in syms.splitlines() if 'getenv' in l]
    csrc = os.path.join(REPO, 'viewformer_amd', 'csrc')
    for f in os.listdir(csrc):
        assert 'getenv' not in open(os.path.join(csrc, f)).read(), f
    n = 6                                                                    # VF_SEL_COUNT (round 6: + VF_SEL_GEMM_TAIL, a bit-identical pair)
    for which in range(n):
        default = 0 if which == 5 else 1                                     # defaults: the faster kernel of each pair IN THE TIMED STEPS (the tail
        assert lib.vf_selected(which) == default                             # policy wins only on isolated launches: off)
        assert lib.vf_select(which, 1 - default) == default and lib.vf_selected(which) == 1 - default
        assert lib.vf_select(which, default) == 1 - default and lib.vf_selected(which) == default
    assert lib.vf_select(n, 1) == -1 and lib.vf_select(-1, 1) == -1 and lib.vf_select(0, 2) == -1 and lib.vf_selected(n) == -1


def test_argument_validation_without_gpu(lib):
    from viewformer_amd._lib import VfIgemmArgs
    P = ctypes.c_void_p
    d = P(4096)            # never dereferenced: validation happens before any launch
    assert lib.vf_igemm_f32(None, None) == -1
    a = VfIgemmArgs()
    assert lib.vf_igemm_f32(ctypes.byref(a), None) == -1
    a.x = a.w_packed = a.out = 4096
    a.M, a.Cin, a.Cout, a.lda, a.ldc = 8, 30, 8, 32, 8
    assert lib.vf_igemm_f32(ctypes.byref(a), None) == -2                  # Cin % 32 != 0 -> unsupported
    a.Cin, a.mode = 32, 7
    assert lib.vf_igemm_f32(ctypes.byref(a), None) == -1
    assert lib.vf_layernorm_f32(d, d, d, d, 4, 6, 1e-5, None) == -2
    assert lib.vf_layernorm_f32(None, d, d, d, 4, 8, 1e-5, None) == -1
    assert lib.vf_vq_argmin_f32(d, d, d, 10, 30, 64, d, None) == -2       # D % 32
    assert lib.vf_vq_argmin_f32(d, d, d, 0, 32, 64, d, None) == 0         # empty input is a no-op
    assert lib.vf_argmax_rows_f32(d, 0, 16, 16, d, None) == 0
    assert lib.vf_argmax_rows_f32(d, 4, 16, 8, d, None) == -1             # ld < n
    assert lib.vf_groupnorm_stats_f32(d, d, 1, 64, 48, 32, 1e-6, d, d, d, None) == -2
    assert lib.vf_attn_blockcausal_f32(d, d, d, d, 1, 2, 64, 64, 64, 128, 128, 128, 1.0, 1, -1, None) == -1   # ldq < H*64
    assert lib.vf_dense_small_k_gelu_f32(d, d, d, d, 4, 32, 8, 1, None) == -2
    assert lib.vf_conv_in_u8_f32(None, None, d, d, d, 1, 8, 8, 32, None) == -1
    # fused output dropout (vf_igemm_args.drop_rate): vf_gemm_bf16's 256-tile shapes only — refused elsewhere, never ignored
    a = VfIgemmArgs()
    a.x = a.w_packed = a.out = 4096
    a.M, a.Cin, a.Cout, a.lda, a.ldc, a.drop_rate = 512, 256, 256, 256, 256, 0.1
    assert lib.vf_igemm_f32(ctypes.byref(a), None) == -2
    assert lib.vf_gemm_x6(ctypes.byref(a), None) == -2 and lib.vf_gemm_x3h(ctypes.byref(a), None) == -2
    assert lib.vf_gemm_bf16(ctypes.byref(a), None) == -2                      # fp32 activations in: no fused form
    a.reserved0, a.drop_row0 = 1, 2
    assert lib.vf_gemm_bf16(ctypes.byref(a), None) == -2                      # drop_row0 % 4 != 0
    assert lib.vf_dropout_add_f32(d, None, d, 4, 0, 0, 0.1, 1, 1, None) == -1  # cols <= 0
    assert lib.vf_dropout_add_f32(d, None, d, 0, 8, 0, 0.1, 1, 1, None) == 0   # empty
    assert lib.vf_dropout_add_f32(d, None, d, 4, 8, 0, 1.0, 1, 1, None) == -1  # rate must be < 1
    # round 6's entries
    assert lib.vf_dense_small_n_f32(d, d, d, d, 0, 1536, 7, 1536, None) == 0                       # empty input is a no-op
    assert lib.vf_dense_small_n_f32(d, d, d, d, 4, 1536, 7, 1000, None) == -1                      # ldx < K
    assert lib.vf_dense_small_n_f32(d, d, d, d, 4, 1536, 9, 1536, None) == -2                      # N > 8: not this kernel's shape
    assert lib.vf_dense_small_n_f32(d, d, d, d, 4, 1534, 7, 1536, None) == -2                      # K % 4
    assert lib.vf_dense_small_n_wgrad_f32(d, d, d, None, 4, 1536, 7, 1536, 0, None) == -1          # no workspace
    assert lib.vf_dense_small_n_wgrad_f32(d, d, d, d, 4, 4096, 7, 4096, 0, None) == -2             # K > 2048
    assert lib.vf_dense_small_n_wgrad_slabs(0) == 0 and lib.vf_dense_small_n_wgrad_slabs(6400) == 400 and lib.vf_dense_small_n_wgrad_slabs(19200) == 600
    assert lib.vf_embed_bwd_f32(d, d, d, d, d, 4, 64, 770, 1026, d, None) == -2                    # d % 4 (rows are read as float4)
    assert lib.vf_embed_bwd_f32(d, d, d, d, d, 4, 64, 768, 1026, None, None) == -1                 # no workspace
    # vf_attn_bwd_bf16: one of its two launches may be skipped (NULL outputs), not both; dK without dV is an error
    z = None
    common = (1, 2, 2, 128, 64, 384, 384, 384, 128, 384, 384, 384, 1.0, -1, 0.0, 0, 0, 0, None)
    assert lib.vf_attn_bwd_bf16(d, d, d, d, d, d, z, z, z, *common) == -1
    assert lib.vf_attn_bwd_bf16(d, d, d, d, d, d, z, d, z, *common) == -1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from viewformer_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_lib.VfError, match='no CPU/PyTorch fallback'):
        _lib.load()


def test_ops_refuse_cpu_tensors(lib):
    import torch
    from viewformer_amd import ops, _lib
    with pytest.raises(_lib.VfError):
        ops.layernorm(torch.zeros(4, 128), torch.ones(128), torch.zeros(128), 4, 128)
    with pytest.raises(_lib.VfError):
        ops.vq_argmin(torch.zeros(4, 32), torch.zeros(8), torch.zeros(8), 32, 64)
