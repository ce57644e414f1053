"""CPU: the framed-tensor helper (tests/framed.py) itself, against torch functions that misbehave on purpose.  Each kind of footprint
violation must be reported with its region, first offset and count — one test per region, so that a ``violations()`` that ignored any
one of them fails here — and a well-behaved function must report nothing.  tests/test_hip_bounds.py proves nothing without this."""
import pytest
import torch

from framed import Frame, FRONT, BACK, ROW_GAP, BATCH_GAP, UNWRITTEN, MODIFIED, ALIGN

CPU = torch.device('cpu')
DTYPES = [torch.float32, torch.bfloat16, torch.uint8, torch.int32, torch.int64, torch.float64]


def _values(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n) % 97 + 1).to(dtype).reshape(shape)


def _good(x, out):
    """a well-behaved kernel: reads and writes logical elements only"""
    out.copy_(x * 2)


@pytest.mark.parametrize('dtype', DTYPES)
def test_layout_alignment_and_guard_size(dtype):
    f = Frame(5, 7, 12, dtype, CPU, batch=2, batch_stride=5 * 12 + 16)
    isz = f.itemsize
    assert f.view.shape == (2, 5, 7) and f.view.stride() == (76, 12, 1)
    assert f.ptr % ALIGN == 0
    assert f.guard * isz >= 1 << 20 and f.start >= f.guard
    assert f.flat.numel() - f.start - f.extent >= f.guard
    wide = Frame(3, 4000, 4096, dtype, CPU)                       # 256 rows x ld outweighs 1 MiB
    assert wide.guard >= 256 * 4096
    # every byte holds the sentinel, and the floating-point ones are NaN
    assert bool((f.ibits == f.sentinel).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(f.flat.float()).all())
    assert f.violations() == [(UNWRITTEN, 0, 2 * 5 * 7)]
    raw = Frame.raw(1000 * isz, CPU, dtype)
    assert raw.view.shape == (1000,) and raw.ptr % ALIGN == 0 and raw.violations() == [(UNWRITTEN, 0, 1000)]


@pytest.mark.parametrize('dtype', DTYPES)
def test_well_behaved_function_reports_nothing(dtype):
    x, out = Frame(6, 5, 9, dtype, CPU), Frame(6, 5, 13, dtype, CPU)
    x.load(_values((6, 5), dtype))
    _good(x.view, out.view)
    assert x.violations() == [] and out.violations() == []
    assert torch.equal(out.logical(), _values((6, 5), dtype) * 2)
    xb, ob = Frame(4, 3, 8, dtype, CPU, batch=3, batch_stride=40), Frame(4, 3, 3, dtype, CPU, batch=3, batch_stride=12)
    xb.load(_values((3, 4, 3), dtype))
    _good(xb.view, ob.view)
    assert xb.violations() == [] and ob.violations() == []


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_element_written_into_a_row_gap(dtype):
    out = Frame(6, 5, 9, dtype, CPU)
    out.view.fill_(1)
    out.widened(6)[2, 5] = 3                                       # column 5 of row 2: the first gap element of that row
    assert out.violations() == [(ROW_GAP, 2 * 9 + 5, 1)]
    assert out.offsets(ROW_GAP).tolist() == [23]
    last = Frame(6, 5, 9, dtype, CPU)
    last.view.fill_(1)
    last.flat[last.start + 5 * 9 + 8] = 3                          # the last gap element of the last row still belongs to the row gap
    assert last.violations() == [(ROW_GAP, 53, 1)]


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_element_written_past_the_last_row(dtype):
    out = Frame(6, 5, 9, dtype, CPU)
    out.view.fill_(1)
    torch.as_strided(out.flat, (7, 5), (9, 1), out.start)[6, 1] = 3     # row 6 of a 6-row output
    assert out.violations() == [(BACK, 6 * 9 + 1, 1)]


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_element_written_before_the_first(dtype):
    out = Frame(6, 5, 9, dtype, CPU)
    out.view.fill_(1)
    out.flat[out.start - 1] = 3
    out.flat[0] = 3                                                # the far end of the guard counts too
    assert out.violations() == [(FRONT, -out.start, 2)]
    assert out.offsets(FRONT).tolist() == [-out.start, -1]


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_element_written_between_batch_entries(dtype):
    out = Frame(4, 3, 8, dtype, CPU, batch=3, batch_stride=40)
    out.view.fill_(1)
    out.flat[out.start + 40 + 4 * 8 + 2] = 3                       # behind the last row of entry 1
    assert out.violations() == [(BATCH_GAP, 40 + 32 + 2, 1)]
    # the same distance behind the LAST entry is the back guard
    out2 = Frame(4, 3, 8, dtype, CPU, batch=3, batch_stride=40)
    out2.view.fill_(1)
    out2.flat[out2.start + 80 + 4 * 8 + 2] = 3
    assert out2.violations() == [(BACK, 80 + 32 + 2, 1)]


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_logical_element_left_unwritten(dtype):
    out = Frame(6, 5, 9, dtype, CPU)
    v = _values((6, 5), dtype)
    for r in range(6):
        for c in range(5):
            if (r, c) != (4, 2):
                out.view[r, c] = v[r, c]
    assert out.violations() == [(UNWRITTEN, 4 * 9 + 2, 1)]
    acc = Frame(6, 5, 9, dtype, CPU).load(v, accumulate=True)      # an accumulating output starts from loaded values: nothing to report
    acc.view.add_(1)
    assert acc.violations() == []


@pytest.mark.parametrize('dtype', DTYPES)
def test_an_input_that_is_written_is_reported(dtype):
    x = Frame(6, 5, 9, dtype, CPU).load(_values((6, 5), dtype))
    x.view[3, 1] += 1
    assert x.violations() == [(MODIFIED, 3 * 9 + 1, 1)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_a_gap_read_that_reaches_the_output_is_seen(dtype):
    """a row sum that runs over the whole stride instead of the logical columns: NaN guards poison the result, and a finite refill changes it"""
    def bad_rowsum(x_view, ld, out):
        rows = x_view.shape[0]
        out.copy_(torch.as_strided(x_view, (rows, ld), (ld, 1)).float().sum(1, keepdim=True).to(out.dtype))

    def good_rowsum(x_view, ld, out):
        out.copy_(x_view.float().sum(1, keepdim=True).to(out.dtype))

    v = _values((6, 5), dtype)
    want = v.float().sum(1, keepdim=True).to(dtype)
    for fn, same in ((good_rowsum, True), (bad_rowsum, False)):
        x, out = Frame(6, 5, 9, dtype, CPU).load(v), Frame(6, 1, 4, dtype, CPU)
        fn(x.view, 9, out.view)
        assert x.violations() == []
        # (under NaN guards the stray read shows in the value; a NaN that propagates may keep the sentinel's payload and then ALSO counts as unwritten)
        assert out.violations() == [] or not same
        assert torch.equal(out.logical().view(out.idtype), want.view(out.idtype)) == same
        for fill in (0.0, 3e38, -3e38):
            x.refill(fill)
            assert x.violations() == []
            out2 = Frame(6, 1, 4, dtype, CPU)
            fn(x.view, 9, out2.view)
            assert torch.equal(out2.logical().view(out2.idtype), want.view(out2.idtype)) == (same or fill == 0.0)


def test_refill_rewrites_everything_outside_the_window_only():
    x = Frame(4, 3, 8, torch.float32, CPU, batch=2, batch_stride=40).load(_values((2, 4, 3), torch.float32))
    x.refill(3e38)
    assert x.violations() == []
    assert torch.equal(x.logical(), _values((2, 4, 3), torch.float32))
    outside = torch.ones(x.flat.numel(), dtype=torch.bool)
    for b in range(2):
        for r in range(4):
            o = x.start + b * 40 + r * 8
            outside[o:o + 3] = False
    assert bool((x.flat[outside] == 3e38).all()) and int(outside.sum()) == x.flat.numel() - 24
    x.flat[x.start + 3] = 0.0                                      # a write into a refilled gap is still a violation
    assert x.violations() == [(ROW_GAP, 3, 1)]


def test_bad_geometry_is_refused():
    for kw in (dict(rows=0, cols=1, ld=1), dict(rows=2, cols=5, ld=4), dict(rows=2, cols=2, ld=4, batch=2, batch_stride=7)):
        with pytest.raises(ValueError):
            Frame(dtype=torch.float32, device=CPU, **kw)
    with pytest.raises(TypeError):
        Frame(2, 2, 2, torch.complex64, CPU)
