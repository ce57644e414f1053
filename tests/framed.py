"""Framed tensors: one allocation = front guard | strided logical window | back guard, every byte a sentinel.

The footprint contract of include/vf_hip.h ("Memory footprint") says a kernel writes exactly the logical elements of its outputs and that
its results depend on the logical elements of its inputs only.  A ``Frame`` makes both observable: the tensor handed to the kernel
(``.view``) is a strided window into a larger buffer whose every other byte holds a recognisable bit pattern, and ``.violations()`` says
where that pattern changed — or where the kernel left it standing inside the window.  The guards are large enough (>= 1 MiB and >= 256 rows)
that an overrun by a whole tile still lands inside the frame's own allocation.

A stray READ shows in the values: a NaN guard that reaches an output makes it NaN (often with the sentinel's own payload, which is then
reported as "unwritten"); selection kernels, whose comparisons ignore NaN, are run again with ``refill(+-3e38)``.

All comparisons are made on integer views of the bits (the floating-point sentinels are NaNs, and NaN != NaN).  Works on CPU tensors too:
tests/test_framed_host.py checks this helper with torch functions that misbehave on purpose.
"""
import torch

FRONT, BACK, ROW_GAP, BATCH_GAP, UNWRITTEN, MODIFIED = 'front guard', 'back guard', 'row gap', 'batch gap', 'unwritten', 'input modified'
_CODE = {FRONT: 1, BACK: 2, ROW_GAP: 3, BATCH_GAP: 4}

# dtype -> (integer dtype of the same width, sentinel bits as a signed value of that dtype)
_S64 = 0xA5A5A5A5A5A5A5A5 - (1 << 64)
_BITS = {
    torch.float32: (torch.int32, 0x7FC0A5A5),                       # quiet NaN, payload 0x00A5A5
    torch.bfloat16: (torch.int16, 0x7FE5),                          # quiet NaN, payload 0x25
    torch.float16: (torch.int16, 0x7EA5),                           # quiet NaN, payload 0xA5
    torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),               # quiet NaN
    torch.uint8: (torch.uint8, 0xA5),
    torch.int32: (torch.int32, 0xA5A5A5A5 - (1 << 32)),
    torch.int64: (torch.int64, _S64),
}
ALIGN = 256
MIN_GUARD_BYTES = 1 << 20
GUARD_ROWS = 256


def _bits_of(value, dtype):
    """the bit pattern of ``value`` stored as ``dtype``, as a Python int of the matching integer dtype"""
    idt, _ = _BITS[dtype]
    return int(torch.tensor([value], dtype=dtype).view(idt)[0])


class Frame:
    def __init__(self, rows, cols, ld, dtype, device, batch=1, batch_stride=None, fill=None, guard_rows=GUARD_ROWS):
        if dtype not in _BITS:
            raise TypeError(f'Frame: no sentinel for {dtype}')
        rows, cols, ld, batch = int(rows), int(cols), int(ld), int(batch)
        batch_stride = rows * ld if batch_stride is None else int(batch_stride)
        if rows < 1 or cols < 1 or ld < cols or batch < 1 or batch_stride < rows * ld:
            raise ValueError(f'Frame: rows {rows}, cols {cols}, ld {ld}, batch {batch}, batch_stride {batch_stride}')
        self.rows, self.cols, self.ld, self.batch, self.batch_stride = rows, cols, ld, batch, batch_stride
        self.dtype, self.device = dtype, torch.device(device)
        self.idtype, self.sentinel = _BITS[dtype]
        isz = torch.empty(0, dtype=dtype).element_size()
        self.itemsize = isz
        guard_bytes = max(MIN_GUARD_BYTES, guard_rows * ld * isz)
        self.guard = (guard_bytes + ALIGN - 1) // ALIGN * ALIGN // isz                # elements, a multiple of 256 bytes
        self.extent = (batch - 1) * batch_stride + rows * ld                        # interior: first logical element .. end of the last row
        slack = ALIGN // isz
        self.flat = torch.empty(self.guard + self.extent + self.guard + slack, dtype=dtype, device=self.device)
        mis = self.flat.data_ptr() % ALIGN
        assert mis % isz == 0
        self.start = self.guard + ((ALIGN - mis) % ALIGN) // isz                     # element index of the interior pointer: 256-byte aligned
        self.guard_bits = self.sentinel
        self.ibits = self.flat.view(self.idtype)
        self.ibits.fill_(self.sentinel)
        if batch == 1:
            self.view = torch.as_strided(self.flat, (rows, cols), (ld, 1), self.start)
        else:
            self.view = torch.as_strided(self.flat, (batch, rows, cols), (batch_stride, ld, 1), self.start)
        assert self.view.data_ptr() % ALIGN == 0
        self._iview = torch.as_strided(self.ibits, self.view.shape, self.view.stride(), self.start)
        self._loaded = None
        self._regions = None
        if fill is not None:
            self.refill(fill)

    @classmethod
    def raw(cls, nbytes, device, dtype=torch.uint8, fill=None):
        """a workspace or packed buffer of exactly ``nbytes`` bytes (``.view`` is the 1-D tensor of ``dtype``)"""
        isz = torch.empty(0, dtype=dtype).element_size()
        if nbytes < 1 or nbytes % isz:
            raise ValueError(f'Frame.raw: {nbytes} bytes of {dtype}')
        f = cls(1, nbytes // isz, nbytes // isz, dtype, device, fill=fill, guard_rows=0)       # (no rows: the guards are 1 MiB each)
        f.view = f.view[0]
        f._iview = f._iview[0]
        return f

    # ------------------------------------------------------------------ geometry
    @property
    def ptr(self):
        return self.view.data_ptr()

    def widened(self, cols):
        """the window with ``cols`` columns per row instead of the declared ones: what a positive control hands to the kernel"""
        assert self.cols <= cols <= self.ld
        shape = (self.rows, cols) if self.batch == 1 else (self.batch, self.rows, cols)
        return torch.as_strided(self.flat, shape, self.view.stride(), self.start)

    def _region_map(self):
        """uint8 code per element of the allocation: 0 logical, else _CODE"""
        if self._regions is None:
            o = torch.arange(self.flat.numel(), device=self.device, dtype=torch.int64) - self.start
            inside = (o >= 0) & (o < self.extent)
            oc = o.clamp(0, max(self.extent - 1, 0))
            in_entry = oc % self.batch_stride
            reg = torch.zeros(self.flat.numel(), dtype=torch.uint8, device=self.device)
            reg[o < 0] = _CODE[FRONT]
            reg[o >= self.extent] = _CODE[BACK]
            reg[inside & (in_entry >= self.rows * self.ld)] = _CODE[BATCH_GAP]
            reg[inside & (in_entry < self.rows * self.ld) & (in_entry % self.ld >= self.cols)] = _CODE[ROW_GAP]
            self._regions = reg
        return self._regions

    # ------------------------------------------------------------------ contents
    def load(self, t, accumulate=False):
        """copy logical values in.  The frame then counts as an INPUT — ``violations()`` reports any logical element whose bits change — unless
        ``accumulate`` says it is a read-modify-write output"""
        t = t.to(device=self.device, dtype=self.dtype)
        self.view.copy_(t.reshape(self.view.shape))
        self._loaded = None if accumulate else self._iview.clone()
        return self

    def refill(self, value):
        """rewrite everything OUTSIDE the logical window (both guards, row gaps, batch gaps) with ``value``"""
        bits = _bits_of(value, self.dtype)
        self.ibits[self._region_map() != 0] = bits
        self.guard_bits = bits
        return self

    def logical(self):
        """a compact copy of the logical window"""
        return self.view.clone()

    def offsets(self, region):
        """sorted element offsets (relative to the interior pointer) of every violation in ``region``"""
        if region == UNWRITTEN:
            bad = self._iview == self.sentinel
        elif region == MODIFIED:
            if self._loaded is None:
                return torch.empty(0, dtype=torch.int64)
            bad = self._iview != self._loaded
        else:
            bad = (self._region_map() == _CODE[region]) & (self.ibits != self.guard_bits)
            return (bad.nonzero().flatten() - self.start).cpu()
        idx = bad.nonzero()
        if idx.numel() == 0:
            return torch.empty(0, dtype=torch.int64)
        strides = torch.tensor(self.view.stride(), dtype=torch.int64, device=idx.device)
        return (idx * strides).sum(1).sort().values.cpu()

    def violations(self):
        """[(region, first offset, count)]: changed bytes in the front guard, back guard, row gaps and batch gaps; and, for a frame that was
        not loaded, logical elements that still hold the sentinel (never written) — for a loaded one, logical elements whose bits changed"""
        out = []
        for region in (FRONT, BACK, ROW_GAP, BATCH_GAP, MODIFIED if self._loaded is not None else UNWRITTEN):
            o = self.offsets(region)
            if o.numel():
                out.append((region, int(o[0]), int(o.numel())))
        return out
