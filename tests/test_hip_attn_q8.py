"""GPU: prefix attention over an e4m3-packed cache (csrc/attention_prefix.hip's Q8 instantiation,
``vf_attn_prefix_q8_bf16``, ``ops.attn_prefix_q8``).

An e4m3 value times a power of two is a bf16 number, and the kernel dequantises a packed tile into the LDS image that the bf16 arm builds
from the unpacked cache: every comparison of the kernel is ``torch.equal`` against ``ops.attn_prefix(ctx_len=, bf16=True)`` on the
dequantised cache, held in the dtype of q.  The packed tiles and scales are made by the restatement (tests/kv_pack_ref.py) on the host —
this file does not depend on the pack kernel — and lie, with the lengths and the output, in ``tests/framed.py`` frames with padded
strides and a gap between the scenes.  The only tolerance is the quantisation itself, held to the project's e4m3 attention bound."""
import numpy as np
import pytest
import torch

import kv_pack_ref as R
from conftest import parity_report
from context_lengths_ref import L, rand, attn_fp64_lengths
from framed import Frame
from test_hip_fp8 import FP8_ATTN_TOL

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 1), (2, 2, 3, 5), (1, 12, 6, 9)]                  # (B, H, C, N): N = 5 leaves a partial group, N = 9 gives three groups
IO = [(torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)]


def case_id(case):
    return 'B%d-H%d-C%d-N%d' % case


def io_id(io):
    n = {torch.bfloat16: 'bf16', torch.float32: 'f32'}
    return f'{n[io[0]]}in-{n[io[1]]}out'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def plan(case):
    """lengths [B,N]: 0, 1, a value in between and C, shifted per scene: every group of four views is mixed"""
    B, H, C, N = case
    cand = sorted({0, 1, C // 2, C} & set(range(C + 1)))
    return np.array([[cand[(n + b) % len(cand)] for n in range(N)] for b in range(B)], dtype=np.int32)


_packed = {}


def packed(case):
    """the context of a case: (values [B, C*L, 3d] fp32, kq / vq uint8 [B, C, H*4096], kscale / vscale [B, C, H], the dequantised cache
    [B, C*L, 3d] fp32 with a zero Q third) — made once per case on the host and left unchanged"""
    if case not in _packed:
        B, H, C, N = case
        d = H * 64
        x = rand((B, C * L, 3 * d), 700 + C, 0.35)
        xf = x.view(B, C, L, 3, H, 64)
        kq, ks = R.pack_tiles(xf[:, :, :, 2].permute(0, 1, 3, 2, 4).contiguous())          # [B, C, H, key, feature]
        vq, vs = R.pack_tiles(xf[:, :, :, 0].permute(0, 1, 3, 4, 2).contiguous())          # [B, C, H, feature, key]
        deq = torch.zeros(B, C, L, 3, H, 64)
        deq[:, :, :, 2] = R.unpack_tiles(kq, ks).permute(0, 1, 3, 2, 4)
        deq[:, :, :, 0] = R.unpack_tiles(vq, vs).permute(0, 1, 4, 2, 3)
        assert torch.equal(deq.bfloat16().float(), deq)
        _packed[case] = (x, kq.view(torch.uint8).reshape(B, C, H * 4096), vq.view(torch.uint8).reshape(B, C, H * 4096), ks, vs,
                         deq.view(B, C * L, 3 * d))
    return _packed[case]


class Setup:
    """frames of one launch; ``bad_from`` [B]: packed views at or beyond it are poisoned (``what``: 'bytes' = 0xFF, 'scales' = NaN)"""

    def __init__(self, dev, case, io, lens, bad_from=None, what=None, q=None):
        B, H, C, N = case
        d = H * 64
        self.case, self.io, self.d = case, io, d
        _, kq, vq, ks, vs, _ = packed(case)
        kq, vq, ks, vs = kq.clone(), vq.clone(), ks.clone(), vs.clone()
        if bad_from is not None:
            for b in range(B):
                if what == 'bytes':
                    kq[b, int(bad_from[b]):] = 0xFF
                    vq[b, int(bad_from[b]):] = 0xFF
                else:
                    ks[b, int(bad_from[b]):] = float('nan')
                    vs[b, int(bad_from[b]):] = float('nan')
        self.q = (rand((B * N * L, 3 * d), 710 + N, 0.35).to(io[0]) if q is None else q).to(dev)
        qv, sv = H * 4096 + 48, H + 1
        one = lambda t: t if B > 1 else t[0]
        self.fk = Frame(C, H * 4096, qv, torch.uint8, dev, batch=B, batch_stride=C * qv + 512).load(one(kq))
        self.fv = Frame(C, H * 4096, qv, torch.uint8, dev, batch=B, batch_stride=C * qv + 512).load(one(vq))
        self.fks = Frame(C, H, sv, torch.float32, dev, batch=B, batch_stride=C * sv + 3).load(one(ks))
        self.fvs = Frame(C, H, sv, torch.float32, dev, batch=B, batch_stride=C * sv + 3).load(one(vs))
        self.fout = Frame(B * N * L, d, d + 8, io[1], dev)
        self.fl = Frame.raw(B * N * 4, dev, dtype=torch.int32).load(torch.from_numpy(lens.reshape(-1).copy()))
        self.frames = (self.fk, self.fv, self.fks, self.fvs, self.fout, self.fl)

    def launch(self):
        from viewformer_amd import ops
        B, H, C, N = self.case
        d, q = self.d, self.q
        ops.attn_prefix_q8(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], self.fk.view, self.fv.view, self.fks.view, self.fvs.view, self.fout.view,
                           B, H, C, N, L, 3 * d, 3 * d, 3 * d, self.fout.ld, self.fl.view, q_view_stride=self.fk.ld,
                           q_scene_stride=self.fk.batch_stride, s_view_stride=self.fks.ld, s_scene_stride=self.fks.batch_stride)
        torch.cuda.synchronize()
        assert [f.violations() for f in self.frames] == [[]] * 6         # exactly the logical output elements; the inputs keep their bits
        return self.fout.logical()


def var_reference(dev, case, io, q, cache, lens, bf16=True, N=None):
    """ops.attn_prefix(ctx_len=) on a plain cache [B, C*L, 3d] held in the dtype of q"""
    from viewformer_amd import ops
    B, H, C, _ = case
    N = case[3] if N is None else N
    d = H * 64
    out = torch.full((B * N * L, d), float('nan'), dtype=io[1], device=dev)
    c0 = cache.to(q.dtype).to(dev).view(B * C * L, 3 * d)
    ops.attn_prefix(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], c0[:, 2 * d:], c0[:, :d], out, B, H, C, N, L, 3 * d, 3 * d, 3 * d, 3 * d, 3 * d,
                    C * L * 3 * d, d, bf16=bf16, ctx_len=torch.from_numpy(lens.reshape(-1).copy()).to(dev))
    return out


@pytest.mark.parametrize('io', IO, ids=io_id)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_a_view_gets_the_bits_of_the_bf16_arm_on_the_dequantised_cache(dev, case, io):
    B, H, C, N = case
    d = H * 64
    lens = plan(case)
    assert {0, C} <= set(lens.flatten().tolist()) or N == 1
    st = Setup(dev, case, io, lens)
    out = st.launch()
    assert not torch.isnan(out.float()).any()
    ref = var_reference(dev, case, io, st.q, packed(case)[5], lens)
    same = bool(torch.equal(out, ref))
    diff = (out.double() - ref.double()).abs().max().item()
    parity_report(test='q8_kernel', case=case_id(case), io=io_id(io), equal=same, max_abs_diff=diff)
    assert same, diff
    # a view launched alone (N = 1) gets its rows of the full launch: the first and the last view of every scene
    for n in sorted({0, N - 1}):
        qn = st.q.view(B, N, L, 3 * d)[:, n].reshape(B * L, 3 * d).contiguous()
        one = Setup(dev, (B, H, C, 1), io, lens[:, n:n + 1], q=qn)
        assert torch.equal(one.launch().view(B, L, d), out.view(B, N, L, d)[:, n]), n


@pytest.mark.parametrize('what', ['bytes', 'scales'])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_packed_views_at_or_beyond_a_views_length_do_not_reach_it(dev, case, what):
    """For every length t that occurs: the packed bytes (0xFF, an e4m3 NaN) or the scales (NaN) of views >= t are poisoned.  A view of
    length <= t reads none of them — although its group stages the poisoned tiles for the longer views next to it — and keeps the bits of
    the clean launch; every longer view reads NaN, which shows that the poison lies where they read."""
    B, H, C, N = case
    d = H * 64
    io = IO[0]
    lens = plan(case)
    clean = Setup(dev, case, io, lens).launch().view(B, N, L, d)
    seen = False
    for t in sorted(set(lens.flatten().tolist())):
        out = Setup(dev, case, io, lens, bad_from=[t] * B, what=what).launch().view(B, N, L, d)
        for b in range(B):
            for n in range(N):
                nan = bool(torch.isnan(out[b, n].float()).any())
                if lens[b, n] <= t:
                    assert not nan and torch.equal(out[b, n], clean[b, n]), (t, b, n)
                else:
                    assert nan, (t, b, n)
                    seen = True
    assert seen or N == 1


@pytest.mark.parametrize('C', [1, 3, 6])
def test_the_quantisation_error_is_inside_the_projects_e4m3_bound_and_above_the_bf16_arms(dev, C):
    """standard normal x 0.35 (the inputs of test_attention_fp8_all_mask_modes), every view at the full length: the error against the
    fp32-equivalent prefix kernel on the UNPACKED data, relative to max |out|, is below FP8_ATTN_TOL (the rounding model alone gives
    5e-2 ... 7e-2 at these C) and above the bf16 arm's own error on the unpacked data (a silent fall-through would be as good as bf16)"""
    case = (2, 4, C, 4)
    B, H, _, N = case
    io = (torch.float32, torch.float32)
    lens = np.full((B, N), C, dtype=np.int32)
    st = Setup(dev, case, io, lens)
    out = st.launch()
    x = packed(case)[0]
    exact = var_reference(dev, case, io, st.q, x, lens, bf16=False)               # the fp32-equivalent arm, unpacked values
    b16 = var_reference(dev, case, io, st.q, x, lens)                             # the bf16 arm, unpacked values
    ref64 = attn_fp64_lengths(x.view(B * C * L, -1), st.q.cpu(), B, H, C, N, lens)
    top = exact.abs().max().item()
    e_q8 = (out - exact).abs().max().item() / top
    e_b16 = (b16 - exact).abs().max().item() / top
    e_ref = (exact.double().cpu() - ref64).abs().max().item() / top
    parity_report(test='q8_accuracy', C=C, err_q8=e_q8, err_bf16=e_b16, err_f32eq_vs_fp64=e_ref, bound=FP8_ATTN_TOL)
    assert e_ref < 1e-4                                                           # the reference is what it claims to be
    assert e_q8 < FP8_ATTN_TOL
    assert e_q8 > e_b16
