"""CPU: the yardstick of tests/test_hip_prefix_bwd.py (tests/prefix_bwd_ref.py) — the float64 reference is pinned against float64
autograd of the oracle's ``compute_attention`` on [prefix; own] keys, wrong kernels are rejected by the bound the GPU test uses, the bound's
constant is calibrated on the fp32 restatement of the kernel, and the new entry validates its arguments before any launch.  No device is
touched."""
import ctypes
import math

import numpy as np
import pytest
import torch

import prefix_bwd_ref as R
from prefix_bwd_ref import CASES, DH, L, case_id


def _pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


# ---------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize('storage', R.STORAGE)
@pytest.mark.parametrize('case', [R.BY_NAME['smallest'], R.BY_NAME['mixed_lengths'], R.BY_NAME['peaked']], ids=case_id)
def test_reference_is_float64_autograd_of_the_oracles_attention(case, storage):
    """per view: keys = [the first c cached views; the view's own], ``compute_attention`` (un-scaled, no mask), loss = sum(out * dout);
    the gradients of the view's own q / k / v are the reference's (dQ, dK, dV); nothing is asked of the cache"""
    from oracle.migt_oracle import compute_attention
    _, (B, H, C, N), _, _ = case
    d = H * DH
    lens = R.lengths_of(case)
    ctx, qkv, dout = R.inputs(case, storage)
    want, mag = R.reference(case, storage)
    got = torch.zeros_like(want)
    for b in range(B):
        for n in range(N):
            c = int(lens[b, n])
            rows = slice((b * N + n) * L, (b * N + n + 1) * L)
            own = qkv[rows].double().view(L, 3, H, DH).permute(1, 2, 0, 3).clone().requires_grad_(True)      # [3][H][L][64]: V, Q, K
            pre = ctx[b, :c * L].double().view(c * L, 3, H, DH).permute(1, 2, 0, 3)
            k = torch.cat([pre[2], own[2]], 1)
            v = torch.cat([pre[0], own[0]], 1)
            out = compute_attention(k, v, own[1])                                                            # [H][L][64]
            (out * dout[rows].double().view(L, H, DH).permute(1, 0, 2)).sum().backward()
            got[rows] = own.grad.permute(2, 0, 1, 3).reshape(L, 3 * d)                                       # columns (V | Q | K)
    assert bool(((got - want).abs() <= 1e-12 * mag).all())
    assert bool((mag > 0).all()) and bool((want.abs() <= mag * (1 + 1e-12)).all())


def test_inputs_have_the_spread_the_cases_name():
    for name, spread in (('mixed_lengths', 1.0), ('peaked', 4.0)):
        case = R.BY_NAME[name]
        ctx, qkv, _ = R.inputs(case)
        d = ctx.shape[-1] // 3
        s = qkv[:L, d:d + DH].double() @ ctx[0, :L, 2 * d:2 * d + DH].double().T
        assert 0.8 * spread < float(s.std()) < 1.25 * spread, (name, float(s.std()))


# ---------------------------------------------------------------------------------------------- 2. calibration, mutants
_CAL = {}


def _calibrated(case, storage):
    key = (case[0], storage)
    if key not in _CAL:
        want, mag = R.reference(case, storage)
        _CAL[key] = (R.worst_ratios(R.restatement(case, storage), want, mag), want, mag)
    return _CAL[key]


def test_calibration():
    """per output: c = 4 x the restatement's worst error / (2^-24 magnitude) over all cases and both storages, rounded up to a power of two"""
    worst = {}
    for case in CASES:
        for storage in R.STORAGE:
            worst[(case[0], storage)] = _calibrated(case, storage)[0]
            print(f'calibration {case[0]} {storage}: restatement worst '
                  + ', '.join(f'{t} {v:.3g}' for t, v in worst[(case[0], storage)].items()) + ' units of 2^-24 x magnitude')
    for t in R.OUTPUTS:
        c = _pow2_ceil(4 * max(w[t] for w in worst.values()))
        print(f'c_{t} = {c:g} (table: {R.C_BOUND[t]:g})')
        assert c == R.C_BOUND[t], (t, worst)


@pytest.mark.parametrize('mut', R.MUTANTS)
def test_mutants_are_rejected(mut):
    """D left out, dK taken from a prefix tile, P without its log-sum-exp, the (V, Q, K) column order swapped: each lies outside the GPU
    test's bounds, by far, on the case with mixed lengths (and the reference itself lies inside: ratio 0).  The subtle one — D from an
    O rounded to bf16 — leaves dV exact and is outside the bounds of dQ and of dK, the outputs whose own constants are two orders
    tighter than dV's."""
    case = R.BY_NAME['mixed_lengths']
    for storage in R.STORAGE:
        _, want, mag = _calibrated(case, storage)
        bad, _ = R.reference(case, storage, mut=mut)
        over = {t: r / R.C_BOUND[t] for t, r in R.worst_ratios(bad, want, mag).items()}
        print(mut, storage, {t: round(v, 2) for t, v in over.items()})
        if mut == 'D_from_bf16_O':
            assert over['dv'] == 0.0 and over['dq'] > 1 and over['dk'] > 1, (storage, over)
        else:
            assert max(over.values()) > 100, (mut, storage, over)
        assert max(R.worst_ratios(want, want, mag).values()) == 0.0


def test_a_views_reference_depends_on_its_own_length_only():
    case = R.BY_NAME['mixed_lengths']
    a, _ = R.reference(case)
    b, _ = R.reference(case, lengths=[[0, 1, 1], [2, 0, 3]])
    v = lambda x, i: x[i * L:(i + 1) * L]
    for i in (0, 2, 3, 5):                                       # views whose length is the same in both
        assert torch.equal(v(a, i), v(b, i))
    for i in (1, 4):
        assert not torch.equal(v(a, i), v(b, i))


# ---------------------------------------------------------------------------------------------- 3. the entry's argument checks
@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _call(lib, q=4096, dout=4096, dqkv=4096, ctx_len=4096, in16=0, B=2, H=12, C=6, N=8, L=64, dh=64, ldq=2304, ldkp=2304, stride=6 * 64 * 2304,
          lddo=768, lddqkv=2304):
    P = ctypes.c_void_p
    ptr = lambda x: None if x is None else P(x)          # never dereferenced: validation happens before any launch
    return lib.vf_attn_prefix_bwd_f32(ptr(q), P(4096), P(4096), P(4096), P(4096), in16, ptr(dout), ptr(dqkv), B, H, C, N, L, dh, ldq, 2304, 2304,
                                      ldkp, 2304, stride, lddo, lddqkv, ptr(ctx_len), None)


def test_the_entry_validates_its_arguments_without_a_device(lib):
    for missing in ('q', 'dout', 'dqkv'):
        assert _call(lib, **{missing: None}) == -1
    assert _call(lib, L=32) == -2                                              # 64-token views only
    assert _call(lib, dh=32) == -2
    assert _call(lib, C=0) == -2                                               # C is the cache's capacity: at least one view
    assert _call(lib, ldq=12 * 64 - 8) == -1                                   # leading dimensions below H * 64 ...
    assert _call(lib, lddo=12 * 64 - 4) == -1
    assert _call(lib, lddqkv=3 * 12 * 64 - 4) == -1                            # ... and below 3 * H * 64 for the (V, Q, K) output
    assert _call(lib, lddo=770) == -1 and _call(lib, lddqkv=2306) == -1        # fp32 rows are written / read as 16-byte vectors
    assert _call(lib, ldkp=2308, N=0) == 0                                     # fp32 storage: multiples of 4 elements
    assert _call(lib, ldkp=2308, N=0, in16=1) == -1                            # bf16 storage: multiples of 8
    assert _call(lib, stride=-2304) == -1
    assert _call(lib, q=4100) == -1 and _call(lib, q=4104) == -1               # fp32 operands: 16-byte aligned bases ...
    assert _call(lib, q=4100, in16=1) == -1 and _call(lib, q=4104, in16=1, N=0) == 0      # ... bf16: 8-byte
    assert _call(lib, dout=4104) == -1 and _call(lib, dqkv=4100) == -1
    assert _call(lib, B=-1) == -1 and _call(lib, N=-1) == -1 and _call(lib, H=0) == -1
    assert _call(lib, N=65536) == -2 and _call(lib, B=65536) == -2             # grid dimensions
    assert _call(lib, N=0) == 0 and _call(lib, B=0) == 0                       # nothing to do: no launch
    assert _call(lib, N=0, ctx_len=None) == 0                                  # NULL lengths: all C views
    assert _call(lib, N=0, q=None) == -1                                       # ... but a missing argument is still refused


def test_the_entry_is_exported_and_the_abi_version_stays(lib):
    from viewformer_amd import _lib
    assert 'vf_attn_prefix_bwd_f32' in _lib.EXPORTS
    var = _lib.EXPORTS['vf_attn_prefix_var_bf16'][1]
    P, I = ctypes.c_void_p, ctypes.c_int
    # the forward's arguments with (dout, dqkv) for (out, out_bf16) and (lddo, lddqkv) for ldo
    assert _lib.EXPORTS['vf_attn_prefix_bwd_f32'][1] == var[:6] + [P, P] + var[8:-3] + [I, I, P, P]
    assert lib.vf_abi_version() == 20


def test_ops_attn_prefix_bwd_refuses_host_tensors(lib):
    from viewformer_amd import ops, _lib
    z = torch.zeros(64, 192)
    with pytest.raises(_lib.VfError):
        ops.attn_prefix_bwd(z[:, 64:128], z[:, 128:], z[:, :64], z[:, 128:], z[:, :64], torch.zeros(64, 64), torch.zeros(64, 192), 1, 1, 1, 1, 64,
                            192, 192, 192, 192, 192, 64 * 192, 64, 192)
