"""GPU: prefix attention over a forked cache (csrc/attention_prefix.hip's ``vf_attn_prefix_fork_*``,
``ops.attn_prefix_fork``): child scene b reads the first split[b] views of parent scene b // share where they lie, then its own views.

The key order and the arithmetic are those of ``vf_attn_prefix_var_*``, so every comparison is ``torch.equal`` against
``ops.attn_prefix(ctx_len=...)`` on a cache materialised here with torch indexing.  Everything the kernel touches — the output, the
lengths, the splits and both segments — lies in ``tests/framed.py`` frames (padded leading dimensions, a gap between the scenes), whose
guards and gaps are NaN: a stray read shows in the values, a stray write in ``violations()``."""
import numpy as np
import pytest
import torch

from conftest import parity_report
from context_lengths_ref import KERNEL_ARMS, L, rand
from framed import Frame

pytestmark = pytest.mark.gpu

# (parent scenes, share, H, C, C2, N): N = 5 leaves a partial group in both arms, N = 9 gives three groups on the bf16 arm
CASES = [(1, 2, 1, 2, 2, 1), (2, 3, 2, 3, 4, 5), (1, 4, 12, 6, 3, 9)]


def case_id(case):
    return 'P%d-S%d-H%d-C%d-O%d-N%d' % case


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def plan(case):
    """(split [B], lengths [B,N]): the splits cycle through 0, C and a value in between; the lengths of a scene cycle through 0, below the
    split, the split, above it and split + C2 (clipped to the valid range), shifted per scene: every group of views is mixed"""
    Bp, S, H, C, C2, N = case
    B = Bp * S
    split = np.array([(0, C, C // 2)[b % 3] for b in range(B)], dtype=np.int32)
    lens = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        s = int(split[b])
        cand = [0, max(s - 1, 0), s, min(s + 1, s + C2), s + C2]
        for n in range(N):
            lens[b, n] = cand[(n + b) % 5]
    return split, lens


def _dt(arm):
    return torch.bfloat16 if arm == 'bf16' else torch.float32


class Setup:
    """frames of one launch; ``parent_from`` [Bp] / ``own_from`` [B]: views at or beyond these are NaN (None: clean)"""

    def __init__(self, dev, arm, case, split, lens, parent_from=None, own_from=None, siblings_alike=False, seed=0):
        Bp, S, H, C, C2, N = case
        B, d, dt = Bp * S, H * 64, _dt(arm)
        self.case, self.arm, self.B, self.d = case, arm, B, d
        par = rand((Bp, C * L, 3 * d), 300 + seed, 0.35).to(dt)
        own = rand((B, C2 * L, 3 * d), 400 + seed, 0.35).to(dt)
        q = rand((B, N * L, 3 * d), 500 + seed, 0.35).to(dt)
        if siblings_alike:                                           # siblings: the same own rows and the same query rows
            own = own.view(Bp, S, C2 * L, 3 * d)[:, :1].expand(Bp, S, C2 * L, 3 * d).reshape(B, C2 * L, 3 * d).contiguous()
            q = q.view(Bp, S, N * L, 3 * d)[:, :1].expand(Bp, S, N * L, 3 * d).reshape(B, N * L, 3 * d).contiguous()
        self.par_clean, self.own_clean = par.clone(), own.clone()
        if parent_from is not None:
            for p in range(Bp):
                par[p, int(parent_from[p]) * L:] = float('nan')
        if own_from is not None:
            for b in range(B):
                own[b, int(own_from[b]) * L:] = float('nan')
        self.q = q.view(B * N * L, 3 * d).to(dev)
        ldp, ldo2 = 3 * d + 16, 3 * d + 32
        self.fp = Frame(C * L, 3 * d, ldp, dt, dev, batch=Bp, batch_stride=C * L * ldp + 64).load(par if Bp > 1 else par[0])
        self.fo2 = Frame(C2 * L, 3 * d, ldo2, dt, dev, batch=B, batch_stride=C2 * L * ldo2 + 128).load(own)
        self.fout = Frame(B * N * L, d, d + 8, dt, dev)
        self.fl = Frame.raw(B * N * 4, dev, dtype=torch.int32).load(torch.from_numpy(lens.reshape(-1).copy()))
        self.fs = Frame.raw(B * 4, dev, dtype=torch.int32).load(torch.from_numpy(split.copy()))
        self.frames = (self.fp, self.fo2, self.fout, self.fl, self.fs)

    def launch(self):
        from viewformer_amd import ops
        Bp, S, H, C, C2, N = self.case
        d, q = self.d, self.q
        p0 = self.fp.view[0] if Bp > 1 else self.fp.view
        o0 = self.fo2.view[0]
        ops.attn_prefix_fork(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], p0[:, 2 * d:], p0[:, :d], o0[:, 2 * d:], o0[:, :d], self.fout.view,
                             self.B, H, C, C2, N, L, 3 * d, 3 * d, 3 * d, self.fp.ld, self.fp.ld, self.fp.batch_stride, self.fo2.ld, self.fo2.ld,
                             self.fo2.batch_stride, self.fout.ld, self.fl.view, self.fs.view, S, bf16=self.arm != 'f32eq')
        torch.cuda.synchronize()
        assert [f.violations() for f in self.frames] == [[]] * 5         # contract 4: exactly the logical output elements, nothing else
        return self.fout.logical()


def materialised(dev, arm, case, split, par, own):
    """[B, (C + C2) L, 3d]: the parent's first split[b] views, the own views behind them, the rest NaN — torch indexing only"""
    Bp, S, H, C, C2, N = case
    B, d = Bp * S, H * 64
    mat = torch.full((B, (C + C2) * L, 3 * d), float('nan'), dtype=_dt(arm))
    for b in range(B):
        s = int(split[b])
        mat[b, :s * L] = par[b // S, :s * L]
        mat[b, s * L:(s + C2) * L] = own[b]
    return mat.to(dev)


def var_reference(dev, arm, case, q, mat, lens, N=None):
    from viewformer_amd import ops
    Bp, S, H, C, C2, _ = case
    N = case[5] if N is None else N
    B, d = Bp * S, H * 64
    out = torch.full((B * N * L, d), float('nan'), dtype=_dt(arm), device=dev)
    m0 = mat.view(B * (C + C2) * L, 3 * d)
    ops.attn_prefix(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], m0[:, 2 * d:], m0[:, :d], out, B, H, C + C2, N, L, 3 * d, 3 * d, 3 * d, 3 * d, 3 * d,
                    (C + C2) * L * 3 * d, d, bf16=arm != 'f32eq', ctx_len=torch.from_numpy(lens.reshape(-1).copy()).to(dev))
    return out


@pytest.mark.parametrize('arm', KERNEL_ARMS)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_a_view_gets_the_bits_of_the_var_entry_on_the_materialised_cache(dev, arm, case):
    """contracts 1 and 4; and view 0 of every scene launched alone (N = 1) gets its rows of the full launch"""
    Bp, S, H, C, C2, N = case
    B, d = Bp * S, H * 64
    split, lens = plan(case)
    assert {0, C} <= set(split.tolist()) and (B < 3 or 0 < split[2] < C)
    st = Setup(dev, arm, case, split, lens)
    out = st.launch()
    assert not torch.isnan(out.float()).any()
    ref = var_reference(dev, arm, case, st.q, materialised(dev, arm, case, split, st.par_clean, st.own_clean), lens)
    same = bool(torch.equal(out, ref))
    diff = (out.double() - ref.double()).abs().max().item()
    parity_report(test='fork_kernel', arm=arm, case=case_id(case), equal=same, max_abs_diff=diff)
    assert same, diff
    # ... and does not depend on share: every child with a parent scene of its own (share = 1) that holds the same rows
    alone = Setup(dev, arm, (B, 1, H, C, C2, N), split, lens)
    alone.fp.load(st.par_clean[torch.arange(B) // S])
    alone.fo2.load(st.own_clean)
    alone.q = st.q
    assert torch.equal(alone.launch(), out)
    one_case = (Bp, S, H, C, C2, 1)
    one = Setup(dev, arm, one_case, split, lens[:, :1])
    one.q = st.q.view(B, N, L, 3 * d)[:, 0].reshape(B * L, 3 * d).contiguous()
    assert torch.equal(one.launch().view(B, L, d), out.view(B, N, L, d)[:, 0])


@pytest.mark.parametrize('arm', KERNEL_ARMS)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_with_share_1_split_C_and_no_own_segment_the_entry_is_the_var_entry(dev, arm, case):
    """contract 2, on the parent frames of the case (B = the parent scenes), own pointers NULL"""
    from viewformer_amd import ops
    Bp, _, H, C, _, N = case
    d, dt = H * 64, _dt(arm)
    lens = np.array([[(n + b) % (C + 1) for n in range(N)] for b in range(Bp)], dtype=np.int32)
    split = np.full(Bp, C, dtype=np.int32)
    st = Setup(dev, arm, (Bp, 1, H, C, 1, N), split, lens)
    p0 = st.fp.view[0] if Bp > 1 else st.fp.view
    q = st.q
    ops.attn_prefix_fork(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], p0[:, 2 * d:], p0[:, :d], None, None, st.fout.view, Bp, H, C, 0, N, L,
                         3 * d, 3 * d, 3 * d, st.fp.ld, st.fp.ld, st.fp.batch_stride, 3 * d, 3 * d, 0, st.fout.ld, st.fl.view, st.fs.view, 1,
                         bf16=arm != 'f32eq')
    torch.cuda.synchronize()
    assert [f.violations() for f in st.frames] == [[]] * 5
    var = torch.full((Bp * N * L, d), float('nan'), dtype=dt, device=dev)
    ops.attn_prefix(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], p0[:, 2 * d:], p0[:, :d], var, Bp, H, C, N, L, 3 * d, 3 * d, 3 * d, st.fp.ld,
                    st.fp.ld, st.fp.batch_stride, d, bf16=arm != 'f32eq', ctx_len=st.fl.view)
    assert torch.equal(st.fout.logical(), var)


@pytest.mark.parametrize('arm', KERNEL_ARMS)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_rows_beyond_the_split_and_beyond_a_views_length_do_not_reach_it(dev, arm, case):
    """contract 3.  For every distinct split t: parent views >= t are NaN, and the own views >= 1 of every scene are NaN.  A view that
    logically reads parent views below t only (min(length, split) <= t) and at most its scene's own view 0 (length <= split + 1) reads
    none of them — although its group stages the NaN tiles for the longer views next to it (lengths are mixed in every group), and
    although a sibling with a larger split reads the same parent scene further — and must have the bits of the clean launch; every
    other view reads NaN, which shows that the poison lies where they read."""
    Bp, S, H, C, C2, N = case
    B, d = Bp * S, H * 64
    split, lens = plan(case)
    clean = Setup(dev, arm, case, split, lens).launch().view(B, N, L, d)
    poisoned_seen = False
    for t in sorted(set(split.tolist())):
        st = Setup(dev, arm, case, split, lens, parent_from=[t] * Bp, own_from=[1] * B)
        out = st.launch().view(B, N, L, d)
        for b in range(B):
            for n in range(N):
                nan = bool(torch.isnan(out[b, n].float()).any())
                if min(lens[b, n], split[b]) <= t and lens[b, n] <= split[b] + 1:      # reads parent views < t and own view 0 at the most
                    assert not nan and torch.equal(out[b, n], clean[b, n]), (t, b, n)
                else:
                    assert nan, (t, b, n)
                    poisoned_seen = True
    assert poisoned_seen or N == 1


@pytest.mark.parametrize('arm', KERNEL_ARMS)
def test_siblings_with_identical_own_rows_return_identical_bits(dev, arm):
    case = CASES[1]
    Bp, S, H, C, C2, N = case
    d = H * 64
    _, lens = plan(case)
    split = np.repeat(np.array([1, C], dtype=np.int32), S)
    lens = np.repeat(np.minimum(lens.reshape(Bp, S, N)[:, 0], split.reshape(Bp, S, 1)[:, 0] + C2), S, 0).astype(np.int32)
    out = Setup(dev, arm, case, split, lens, siblings_alike=True).launch().view(Bp, S, N * L, d)
    assert not torch.isnan(out.float()).any()
    for s in range(1, S):
        assert torch.equal(out[:, s], out[:, 0]), s
