"""The row driver of the three encoders (mg_format_calls, mg_encode_calls_bcf, mg_format_site_info) on the directed cases of
tests/row_cases.py -- a value on every seam of window, tile, capacity, descriptor and power of ten; tests/test_row_cases_cpu.py proves
that each case holds what it claims -- and the driver's scan by itself (mg_debug_row_scan) where the offsets pass 2^32, which no
encoder reaches at test size.  The expected bytes are those of the plain formatters of the existing test files; every comparison is
exact."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import row_cases as rc
from malva_amd import Context
from malva_amd.capi import CELLS_GP, CELLS_PL, BcfKeys, Cells

pytestmark = pytest.mark.gpu
MG_ERR_LIMIT = -5
FRONT, BEHIND, FILL = 64, 4096, 0xAA


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def _pad(a):
    return np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))


class _Entry:
    """a case's two entries with their arguments bound: call(device, out, cap, row_off) -> (rc, bytes needed)"""

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        a = case.arrays()
        f = case.fields
        if case.encoder == "info":
            used = ("ac", "ns", "vao")
        else:
            lists = bool(f & {"GP", "PL"})
            used = ("gt1", "gt2", "gq") + (("cov",) if "COVS" in f else ()) + (("vao",) if lists or "COVS" in f else ()) + (("vgo",) if lists else ()) \
                + (("probs", "status") if "GP" in f else ()) + (("pl",) if "PL" in f else ())
        self.host = {k: _pad(a[k]) for k in used}
        self.dev = {k: torch.from_numpy(v.reshape(-1).view(np.uint8)).to(torch.device("cuda", 0)) for k, v in self.host.items()}
        torch.cuda.synchronize()

    def call(self, device, out, cap, row_off):
        c, L, h = self.case, self.ctx._L, self.ctx.h
        ptr = (lambda k: self.dev[k].data_ptr() if k in self.dev else None) if device else (lambda k: self.host[k].ctypes.data if k in self.host else None)
        need = C.c_uint64(0)
        tail = (C.c_void_p(out if cap else None), cap, C.c_void_p(row_off), C.byref(need))
        if c.encoder == "info":
            rc_ = (L.mg_format_site_info_device if device else L.mg_format_site_info)(h, c.n, ptr("ac"), ptr("ns"), ptr("vao"), *tail)
        else:
            cells = Cells(c.n, c.planes, int(c.haploid), ptr("gt1"), ptr("gt2"), ptr("gq"), int(c.min_gq is not None), int(c.min_gq or 0), ptr("cov"), ptr("vao"),
                          ptr("probs"), ptr("vgo"), ptr("status"), ptr("pl"), None, (CELLS_GP if "GP" in c.fields else 0) | (CELLS_PL if "PL" in c.fields else 0))
            if c.encoder == "text":
                rc_ = (L.mg_format_calls_device if device else L.mg_format_calls)(h, C.byref(cells), *tail)
            else:
                rc_ = (L.mg_encode_calls_bcf_device if device else L.mg_encode_calls_bcf)(h, C.byref(cells), C.byref(BcfKeys(*c.keys)), *tail)
        if device:
            self.ctx.synchronize()
        return rc_, need.value

    def run(self, device, cap):
        """-> (rc, needed, guard in front, the cap bytes, guard behind, row_off) with the buffer `shift` past a 16-byte aligned address"""
        c = self.case
        size = FRONT + c.shift + cap + BEHIND
        if device:
            buf = torch.full((size,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
            off = torch.full((c.n + 1,), -1, dtype=torch.int64, device=buf.device)
            torch.cuda.synchronize()
            assert buf.data_ptr() % 16 == 0, "the allocation is not 16-byte aligned: the case's misalignment would not be its shift"
            rc_, need = self.call(True, buf.data_ptr() + FRONT + c.shift, cap, off.data_ptr())
            got, got_off = buf.cpu().numpy(), off.cpu().numpy().view(np.uint64)
        else:
            raw = np.full(size + 16, FILL, dtype=np.uint8)
            lead = -raw.ctypes.data % 16
            got = raw[lead:lead + size]
            got_off = np.full(c.n + 1, 1 << 63, dtype=np.uint64)
            rc_, need = self.call(False, got.ctypes.data + FRONT + c.shift, cap, got_off.ctypes.data)
        at = FRONT + c.shift
        return rc_, need, got[:at], got[at:at + cap].tobytes(), got[at + cap:], got_off


@pytest.mark.parametrize("case", rc.cases(), ids=lambda c: c.name)
def test_case(ctx, case):
    want, want_off = case.expected()
    entry = _Entry(ctx, case)
    for device in (False, True):
        rc_, need, front, got, behind, off = entry.run(device, len(want))
        assert rc_ == 0 and need == len(want), (device, rc_, need)
        assert np.array_equal(off, want_off)
        assert got == want, "first difference at byte %d" % next(i for i, (x, y) in enumerate(zip(got, want)) if x != y)
        assert (front == FILL).all(), "bytes in front of the buffer were written"
        assert (behind == FILL).all(), "bytes behind the buffer were written"
        for cap in case.caps:
            rc_, need, front, got, behind, off = entry.run(device, cap)
            assert rc_ == MG_ERR_LIMIT and need == len(want), (device, cap, rc_, need)
            assert np.array_equal(off, want_off), "row_off is not whole at capacity %d" % cap
            assert (behind == FILL).all(), "bytes at or behind capacity %d were written" % cap
            assert (front == FILL).all(), "bytes in front of the buffer were written at capacity %d" % cap
            assert got == want[:cap], "the bytes in front of capacity %d are not the output's first" % cap
            rc_, need2, front, got, behind, off = entry.run(device, need)
            assert rc_ == 0 and need2 == need and got == want and (front == FILL).all() and (behind == FILL).all()


# ---- the scan by itself: row_off in 64 bits where the lengths add up past 2^32 ----------------------------------------------------

@pytest.mark.parametrize("n", rc.SCAN_N)
def test_row_scan(ctx, n):
    for name, lens in rc.scan_inputs(n):
        want = [0] + list(itertools.accumulate(int(x) for x in lens))
        off, total = ctx.row_scan(lens)
        assert [int(x) for x in off] == want, (name, next(i for i, (x, y) in enumerate(zip(off, want)) if int(x) != y))
        assert total == want[-1], name
        off, total = ctx.row_scan(lens, flag=True)                               # a length pass met a row of 4 GB or more
        assert [int(x) for x in off] == want, name
        assert total == ((1 << 64) - 1 if n else 0), name
    if n >= 3:
        assert want[-1] != 0 and rc.scan_inputs(n)[0][1].sum(dtype=np.uint64) >= 1 << 32


def test_row_scan_leaves_the_encoders_alone(ctx):
    """the debug entry shares the text encoder's scratch: an encoder call behind it is what it was"""
    case = next(c for c in rc.cases() if c.name == "text-rows-33")
    want, want_off = case.expected()
    ctx.row_scan(np.full(20000, rc.U32_MAX, dtype=np.uint32), flag=True)
    rc_, need, front, got, behind, off = _Entry(ctx, case).run(False, len(want))
    assert rc_ == 0 and got == want and np.array_equal(off, want_off)
