"""GPU: the mean-view row kernel (csrc/mix_rows.hip, ops.mix_rows) — the five contracts of include/vf_hip.h's entry over the case table of
tests/mix_kernels_ref.py (pinned on the CPU by tests/test_mix_ref_host.py):
  A  top_k = 1 on a unique maximum is ops.codebook_gather of the arg-max, bit for bit;
  B  kept / thr are ops.sample_rows' on the same logits and parameters, torch.equal, in every case;
  C  a row's outputs are the same bits alone or among others, at any number of rows, whatever outputs are requested, compact or padded;
  D  in framed buffers exactly rows x D elements of out and rows of kept / thr are written and only the columns 0 .. N-1 of the logits
     and of E are read (+3e38 behind the logits, NaN behind E);
  E  out is within c x 2^-24 x magnitude of the float64 reference evaluated on the kept set the device reports (the sampler's, by B),
     element by element, c = M.C_OUT's: 4 x the float32 restatement's worst deviation, never a figure taken from the kernel.
The exact class (all-equal rows, integer codebook) must equal float64 exactly."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import mix_kernels_ref as M
import sample_kernels_ref as R
from conftest import parity_report
from framed import Frame

pytestmark = pytest.mark.gpu

C = M.C_OUT[1]
OUT = ('out', 'kept', 'thr')
RG = M.ROWS_PER_GROUP
_worst = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    from viewformer_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    for k in sorted(_worst):
        parity_report(test='mix_rows', what=k, c=C, **_worst[k])


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f'{what}: {k} differs in its bits'


def _run(dev, case, x, E, want=OUT):
    from viewformer_amd import ops
    rows, N, D, T, top_k, top_p, padded, shift = case
    xd = x.to(dev) if padded else x[:, :N].contiguous().to(dev)
    Ed = E.to(dev) if padded else E[:, :N].contiguous().to(dev)
    return ops.mix_rows(xd, rows, N, Ed, D, temperature=T, top_k=top_k, top_p=top_p, ld=N + R.PAD if padded else None,
                        ldE=N + M.PAD_E if padded else None, want=want)


# ------------------------------------------------------------------ B and E over the case table
@pytest.mark.parametrize('N', M.NS)
def test_the_kernel_against_the_reference_and_the_sampler(dev, N):
    """every (top_k, top_p) of the lists at this N; rows 1 / 3 / R-1 / R / R+1 / 2R+1, D 32 / 256, T 0.5 / 1 / 2, compact and padded
    operands walk with the case; rows of every kind of R.KINDS, the all -inf row among them"""
    from viewformer_amd import ops
    worst, elements = 0.0, 0
    for case in M.cases(N):
        rows, _, D, T, top_k, top_p, padded, shift = case
        x, E, kinds = M.inputs_for(case)
        got = _run(dev, case, x, E)
        assert got['out'].dtype == torch.float32 and tuple(got['out'].shape) == (rows, D) and got['kept'].dtype == torch.int32
        # B: the sampler's set, bit for bit
        smp = ops.sample_rows(x.to(dev), rows, N, temperature=T, top_k=top_k, top_p=top_p, ld=N + R.PAD, want=('kept', 'thr'))
        assert torch.equal(got['kept'], smp['kept']) and torch.equal(_bits(got['thr']), _bits(smp['thr'])), case
        # the all -inf row
        kept = got['kept'].cpu().numpy()
        for r, kind in enumerate(kinds):
            if kind == 'all_neg_inf':
                assert kept[r] == 0 and bool(torch.isnan(got['thr'][r])) and bool(torch.isnan(got['out'][r]).all()), case
            else:
                assert kept[r] >= 1 and bool(torch.isfinite(got['out'][r]).all()), (case, r, kind)
        # E: float64 on the set the device reports
        z = x[:, :N].numpy()
        ref = M.mix_ref(z, E[:, :N].numpy(), T, top_k, top_p, keep=M.keep_from_count(z, kept))
        w = M.worst_ratio(got['out'], ref)
        print(f'{case}: worst {w:.3f} x 2^-24 x magnitude')
        assert w <= C, (case, w)
        worst, elements = max(worst, w), elements + rows * D
    _worst[f'N {N}'] = dict(elements=elements, worst=round(worst, 3))


# ------------------------------------------------------------------ A
@pytest.mark.parametrize('N,D', [(1, 32), (63, 32), (65, 256), (128, 32), (1024, 256)])
def test_top_k_1_is_the_codebook_gather_of_the_argmax(dev, N, D):
    from viewformer_amd import ops
    rows = 2 * RG + 1
    x, kinds, _ = R.inputs(rows, N, shift=0)
    z = x[:, :N]
    unique = ((z == z.max(1, keepdim=True).values).sum(1) == 1) & torch.isfinite(z.max(1).values)
    assert int(unique.sum()) >= 15
    xd, Ed = x.to(dev), M.codebook(D, N)[:, :N].contiguous().to(dev)
    am = ops.argmax_rows(xd, rows, N, ld=N + R.PAD)
    want = ops.codebook_gather(Ed, am, D, N)
    u = unique.to(dev)
    for T, top_p in ((1.0, 1.0), (0.5, 0.9), (2.0, 1e-6)):
        got = ops.mix_rows(xd, rows, N, Ed, D, temperature=T, top_k=1, top_p=top_p, ld=N + R.PAD, want=OUT)
        assert bool((got['kept'][u] == 1).all())
        assert torch.equal(_bits(got['out'][u]), _bits(want[u])), (N, D, T)
    # a nucleus so small that it is the maximum alone: the same
    got = ops.mix_rows(xd, rows, N, Ed, D, top_p=1e-6, ld=N + R.PAD)
    assert torch.equal(_bits(got['out'][u]), _bits(want[u]))


# ------------------------------------------------------------------ the exact class
@pytest.mark.parametrize('case', M.exact_cases())
def test_the_exact_class_equals_float64(dev, case):
    from viewformer_amd import ops
    rows, N, D, T, top_k, top_p = case
    z, E, ref = M.exact_inputs(case)
    got = ops.mix_rows(z.to(dev), rows, N, E.to(dev), D, temperature=T, top_k=top_k, top_p=top_p, ldE=N + M.PAD_E, want=OUT)
    assert bool((got['kept'] == N).all()) and bool((got['thr'] == float(np.float32(1.5) / np.float32(T))).all())
    assert np.array_equal(got['out'].cpu().numpy().astype(np.float64), ref['out']), case


# ------------------------------------------------------------------ C
@pytest.mark.parametrize('N,D', [(65, 32), (1024, 256)])
def test_a_rows_outputs_depend_on_nothing_but_the_row(dev, N, D):
    from viewformer_amd import _lib, ops
    rows, T, top_k, top_p = 2 * RG + 1, 0.5, 64, 0.9
    x, kinds, _ = R.inputs(rows, N, shift=3)
    E = M.codebook(D, N)
    xd, xc, Ed, Ec = x.to(dev), x[:, :N].contiguous().to(dev), E.to(dev), E[:, :N].contiguous().to(dev)
    kw = dict(temperature=T, top_k=top_k, top_p=top_p)
    full = ops.mix_rows(xd, rows, N, Ed, D, ld=N + R.PAD, ldE=N + M.PAD_E, want=OUT, **kw)
    _same_bits(ops.mix_rows(xd, rows, N, Ed, D, ld=N + R.PAD, ldE=N + M.PAD_E, want=OUT, **kw), full, 'second launch')
    _same_bits(ops.mix_rows(xc, rows, N, Ec, D, want=OUT, **kw), full, 'compact')
    # every row alone against the same row among 2R+1: other kinds of rows keep other tiles, and the row sits in another MFMA column
    for r in range(rows):
        alone = ops.mix_rows(xc[r:r + 1], 1, N, Ec, D, want=OUT, **kw)
        _same_bits(alone, {k: v[r:r + 1] for k, v in full.items()}, f'row {r} ({kinds[r]}) alone')
    # any number of rows: prefixes and a suffix that starts inside a workgroup
    for n in (3, RG - 1, RG, RG + 1):
        _same_bits(ops.mix_rows(xc[:n], n, N, Ec, D, want=OUT, **kw), {k: v[:n] for k, v in full.items()}, f'first {n} rows')
    _same_bits(ops.mix_rows(xc[5:], rows - 5, N, Ec, D, want=OUT, **kw), {k: v[5:] for k, v in full.items()}, 'rows 5 ...')
    # every combination of outputs
    for n in range(1, 4):
        for want in itertools.combinations(OUT, n):
            got = ops.mix_rows(xc, rows, N, Ec, D, want=want, **kw)
            assert tuple(got) == want
            _same_bits(got, {k: full[k] for k in want}, f'want {want}')
    # a padded ldo (the C entry; ops allocates compact outputs)
    ldo = D + 5
    fo = torch.full((rows, ldo), 7.0, device=dev)
    P = ctypes.c_void_p
    st = _lib.load().vf_mix_rows_f32(P(xc.data_ptr()), rows, N, N, T, top_k, top_p, P(Ec.data_ptr()), D, N, P(fo.data_ptr()), ldo, None, None, _strm())
    assert st == 0
    assert torch.equal(_bits(fo[:, :D].contiguous()), _bits(full['out'])) and bool((fo[:, D:] == 7.0).all())


# ------------------------------------------------------------------ D
@pytest.mark.parametrize('rows,N,D', [(RG + 3, 1000, 256), (5, 63, 32)])
def test_the_kernel_writes_only_its_outputs_and_reads_only_its_inputs(dev, rows, N, D):
    """framed buffers (tests/framed.py): the logits' pad and guards hold NaN, then +3e38 (a read past N wins the row), then -3e38; E's pad
    and guards hold NaN throughout (a read past N poisons the output); every output in a frame of its own, out with a padded ldo"""
    from viewformer_amd import _lib, ops
    x, kinds, _ = R.inputs(rows, N, shift=0)
    E = M.codebook(D, N)
    T, top_k, top_p = 2.0, 64, 0.9
    want = ops.mix_rows(x[:, :N].contiguous().to(dev), rows, N, E[:, :N].contiguous().to(dev), D, temperature=T, top_k=top_k, top_p=top_p, want=OUT)
    fx = Frame(rows, N, N + R.PAD, torch.float32, dev).load(x[:, :N])
    fe = Frame(D, N, N + M.PAD_E, torch.float32, dev).load(E[:, :N])
    outs = dict(out=Frame(rows, D, D + 7, torch.float32, dev), kept=Frame(1, rows, rows, torch.int32, dev), thr=Frame(1, rows, rows, torch.float32, dev))
    P = ctypes.c_void_p
    for fill in (None, 3e38, -3e38):
        if fill is not None:
            fx.refill(fill)
            for f in outs.values():
                f.ibits.fill_(f.sentinel)
        st = _lib.load().vf_mix_rows_f32(P(fx.ptr), rows, N, N + R.PAD, T, top_k, top_p, P(fe.ptr), D, N + M.PAD_E, P(outs['out'].ptr), D + 7,
                                         P(outs['kept'].ptr), P(outs['thr'].ptr), _strm())
        assert st == 0
        torch.cuda.synchronize()
        for name, f in [('logits', fx), ('E', fe)] + list(outs.items()):
            assert f.violations() == [], (name, fill, f.violations())
        _same_bits({k: outs[k].logical().view(want[k].shape) for k in OUT}, want, f'framed, guards {fill}')


def test_refusals_reach_the_caller(dev):
    from viewformer_amd import _lib, ops
    z, E = torch.zeros((2, 64), device=dev), torch.zeros((32, 64), device=dev)
    for bad in (dict(temperature=-1.0), dict(top_p=0.0), dict(top_k=-1)):
        with pytest.raises(_lib.VfError):
            ops.mix_rows(z, 2, 64, E, 32, **bad)
    with pytest.raises(_lib.VfError):
        ops.mix_rows(z, 2, 64, torch.zeros((48, 64), device=dev), 48)
    with pytest.raises(ValueError):
        ops.mix_rows(z, 3, 64, E, 32)
    with pytest.raises(ValueError):
        ops.mix_rows(z, 2, 64, E[:16], 32)
    assert tuple(ops.mix_rows(z[:0], 0, 64, E, 32)['out'].shape) == (0, 32)
