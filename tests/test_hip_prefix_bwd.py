"""GPU: the backward of the prefix-cache attention over the query views (csrc/attention_prefix_bwd.hip, ``ops.attn_prefix_bwd``) against
the float64 reference of the values as stored (tests/prefix_bwd_ref.py): every output within ``C_BOUND[output] * 2^-24 * magnitude``, the
constants (one each for dV, dQ, dK) calibrated on the CPU restatement of the kernel (tests/test_prefix_bwd_ref_host.py), never on the kernel.  All buffers are
``tests/framed.py`` frames: padded leading dimensions, a gap between the scenes of the cache, NaN sentinels everywhere else.  The exact
part of the contract — a view's bits do not depend on N, its position, the other views' lengths, the capacity or on cache rows beyond its
length — is ``torch.equal``.  Every measured worst ratio goes to the parity report (profiles/prefix_bwd_parity.txt)."""
import numpy as np
import pytest
import torch

import prefix_bwd_ref as R
from conftest import parity_report
from framed import Frame
from prefix_bwd_ref import CASES, DH, L, case_id

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


class _Buffers:
    """frames of one case: the query rows' qkv (ld 3d + 8), the cache (ld 3d + 16, scenes a gap apart), dout (ld d + 4), the lengths, and
    the output dqkv (ld 3d + 12)"""

    def __init__(self, dev, case, storage, poison_from=None, lengths='case'):
        _, (B, H, C, N), _, _ = case
        d = H * DH
        self.B, self.H, self.C, self.N, self.d = B, H, C, N, d
        dt = torch.bfloat16 if storage == 'bf16' else torch.float32
        ctx, qkv, dout = R.inputs(case, storage)
        if poison_from is not None:                                  # cache views >= poison_from are NaN
            ctx = ctx.clone()
            ctx[:, poison_from * L:] = float('nan')
        ldp = 3 * d + 16
        self.fc = Frame(C * L, 3 * d, ldp, dt, dev, batch=B, batch_stride=C * L * ldp + 64).load(ctx if B > 1 else ctx[0])
        self.fq = Frame(B * N * L, 3 * d, 3 * d + 8, dt, dev).load(qkv)
        self.fd = Frame(B * N * L, d, d + 4, torch.float32, dev).load(dout)
        self.fo = Frame(B * N * L, 3 * d, 3 * d + 12, torch.float32, dev)
        lens = R.lengths_of(case) if isinstance(lengths, str) else lengths
        self.fl = None if lens is None else Frame.raw(B * N * 4, dev, dtype=torch.int32).load(torch.as_tensor(np.asarray(lens), dtype=torch.int32).reshape(-1))

    def launch(self, C=None):
        from viewformer_amd import ops
        d, q = self.d, self.fq.view
        c0 = self.fc.view[0] if self.B > 1 else self.fc.view
        ops.attn_prefix_bwd(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], c0[:, 2 * d:], c0[:, :d], self.fd.view, self.fo.view, self.B, self.H,
                            self.C if C is None else C, self.N, L, self.fq.ld, self.fq.ld, self.fq.ld, self.fc.ld, self.fc.ld, self.fc.batch_stride,
                            self.fd.ld, self.fo.ld, ctx_len=None if self.fl is None else self.fl.view)
        torch.cuda.synchronize()
        return self

    def untouched(self):
        frames = [self.fc, self.fq, self.fd, self.fo] + ([] if self.fl is None else [self.fl])
        return [v for f in frames for v in f.violations()]


_REF = {}


def _reference(case, storage):
    """computed once per (case, storage), shared and left unchanged"""
    key = (case[0], storage)
    if key not in _REF:
        _REF[key] = R.reference(case, storage)
    return _REF[key]


@pytest.mark.parametrize('storage', R.STORAGE)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_every_output_within_the_calibrated_bound_of_float64(dev, case, storage):
    """... and the kernel writes exactly the logical elements of dqkv: every one of them, nothing else, no input changed.  The case with
    scene lengths 2 of 4 has its unfilled cache rows set to NaN."""
    name, (B, H, C, N), _, _ = case
    want, mag = _reference(case, storage)
    bufs = _Buffers(dev, case, storage, poison_from=2 if name == 'scene_lengths' else None).launch()
    assert bufs.untouched() == []
    got = bufs.fo.logical().cpu()
    assert not torch.isnan(got).any()
    ratios = R.worst_ratios(got, want, mag)
    parity_report(test='prefix_bwd_kernel', case=name, storage=storage, B=B, H=H, C=C, N=N, lengths=R.lengths_of(case).tolist(),
                  unit='2^-24 x magnitude', bound=R.C_BOUND, **{'worst_' + k: v for k, v in ratios.items()})
    for t in R.OUTPUTS:
        assert ratios[t] <= R.C_BOUND[t], (t, ratios)


@pytest.mark.parametrize('storage', R.STORAGE)
def test_view_3_alone_has_the_bits_of_view_3_among_four(dev, storage):
    case = R.BY_NAME['scene_lengths']
    _, (B, H, C, N), _, _ = case
    d = H * DH
    four = _Buffers(dev, case, storage).launch().fo.logical().view(B, N, L, 3 * d)
    one = _Buffers(dev, case, storage)
    # the same buffers, N = 1: scene b's only view is view 3 of the full launch
    from viewformer_amd import ops
    for b in range(B):
        rows = one.fq.view[(b * N + 3) * L:(b * N + 4) * L]
        c0 = one.fc.view[b]
        out = torch.full((L, 3 * d), float('nan'), dtype=torch.float32, device=dev)
        ops.attn_prefix_bwd(rows[:, d:2 * d], rows[:, 2 * d:], rows[:, :d], c0[:, 2 * d:], c0[:, :d], one.fd.view[(b * N + 3) * L:(b * N + 4) * L],
                            out, 1, H, C, 1, L, one.fq.ld, one.fq.ld, one.fq.ld, one.fc.ld, one.fc.ld, one.fc.batch_stride, one.fd.ld, 3 * d,
                            ctx_len=one.fl.view[b * N + 3:b * N + 4])
        torch.cuda.synchronize()
        assert torch.equal(out, four[b, 3]), b


@pytest.mark.parametrize('storage', R.STORAGE)
def test_a_length_c_has_the_bits_of_capacity_c_and_no_lengths_means_all(dev, storage):
    """``ctx_len = c`` for every view == ``C = c`` without lengths, on the same buffers and prefix_stride; NULL lengths == all-C lengths;
    and a view's bits do not depend on the other views' lengths (the mixed case against the uniform ones)"""
    case = R.BY_NAME['mixed_lengths']
    _, (B, H, C, N), _, _ = case
    d = H * DH
    mixed = _Buffers(dev, case, storage).launch().fo.logical().view(B * N, L, 3 * d)
    lens = R.lengths_of(case).reshape(-1)
    for c in range(1, C + 1):
        by_len = _Buffers(dev, case, storage, lengths=np.full((B, N), c)).launch()
        by_cap = _Buffers(dev, case, storage, lengths=None).launch(C=c)
        assert by_len.untouched() == [] and by_cap.untouched() == []
        a, b = by_len.fo.logical(), by_cap.fo.logical()
        assert torch.equal(a, b), c
        sel = torch.from_numpy(lens == c).to(dev)
        assert bool(sel.any()) and torch.equal(mixed[sel], a.view(B * N, L, 3 * d)[sel]), c
    none = _Buffers(dev, case, storage, lengths=None).launch().fo.logical()
    full = _Buffers(dev, case, storage, lengths=np.full((B, N), C)).launch().fo.logical()
    over = _Buffers(dev, case, storage, lengths=np.full((B, N), C + 5)).launch().fo.logical()     # clamped to the capacity on read
    assert torch.equal(none, full) and torch.equal(over, full)
    zero = _Buffers(dev, case, storage, lengths=np.zeros((B, N))).launch().fo.logical().view(B * N, L, 3 * d)
    sel = torch.from_numpy(lens == 0).to(dev)
    assert bool(sel.any()) and torch.equal(mixed[sel], zero[sel])


@pytest.mark.parametrize('storage', R.STORAGE)
def test_cache_rows_beyond_a_views_length_are_not_read(dev, storage):
    """scene lengths 2 of capacity 4: the bits with NaN in the unfilled rows are the bits with numbers there"""
    case = R.BY_NAME['scene_lengths']
    clean = _Buffers(dev, case, storage).launch().fo.logical()
    dirty = _Buffers(dev, case, storage, poison_from=2).launch()
    assert torch.isnan(dirty.fc.view[:, 2 * L:].float()).all()
    assert torch.equal(dirty.fo.logical(), clean)
