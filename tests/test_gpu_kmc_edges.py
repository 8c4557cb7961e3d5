"""kmc_decode_kernel behind mg_kmc_set_lut / mg_kmc_decode_records / mg_kmc_scan_records on the directed cases of tests/kmc_cases.py:
record shapes up to k = 64, runs of every length around a tile, the 512-entry window's edge, bins that end inside a tile or hold
nothing, the table's end, the count filter at its bounds, a table set over another, the scan's two runs and the HOST_PIECE seam.
The expected rows are the items each case was written from; everything is exact.  tests/test_kmc_cases_cpu.py proves, without a
GPU, that each case holds what its name says."""
import numpy as np
import pytest

import kmc_cases as kc
from malva_amd import BF_ALT, BF_CTX, Context
from malva_amd.capi import rows_of
from oracle import capi as ocapi

pytestmark = pytest.mark.gpu


def _set(ctx, c):
    ctx.kmc_set_lut(c.lut, c.p, c.sb, c.cb, c.min_count, c.max_count, c.total)


def _check_runs(ctx, c):
    for first, n in c.runs:
        hi, lo, cnt = ctx.kmc_decode_records(c.records[first:first + n], first_record=first)
        for what, got, want in (("hi", hi, c.hi), ("lo", lo, c.lo), ("cnt", cnt, c.cnt)):
            bad = np.flatnonzero(got != want[first:first + n])
            assert bad.size == 0, (c.name, (first, n), what, bad[:5], got[bad[:5]], want[first:first + n][bad[:5]])


@pytest.mark.parametrize("name", kc.case_ids())
def test_decode_case(name):
    c = kc.case(name)
    with Context(min(c.k, 35), c.k, 1 << 20) as ctx:
        _set(ctx, c)
        _check_runs(ctx, c)


def test_a_second_smaller_table_replaces_the_first():
    """one context (its ref_k is the databases' k = 11): a table of 2 x 4^7 entries with records of 2 bytes, then one of 2 x 4^3
    entries with records of 6 bytes and other count bounds, then the first again"""
    a, b = kc.case("first-table-k11"), kc.case("count-u32-max-2^40")
    assert a.k == b.k == 11 and len(b.lut) < len(a.lut) and (a.sb + a.cb, b.sb + b.cb) == (2, 6) and (a.p, b.p) == (7, 3)
    assert (a.min_count, a.max_count) != (b.min_count, b.max_count)
    with Context(11, 11, 1 << 20) as ctx:
        for c in (a, b, a):
            _set(ctx, c)
            _check_runs(ctx, c)


def test_scan_from_two_runs_of_records_equals_the_oracle_scan_of_the_items():
    c = kc.case("scan-43")
    k, ref_k, bits = 35, 43, 1 << 20
    val = [(int(h) << 64) | int(l) for h, l in zip(c.hi, c.lo)]
    text = [bytes(b"ACGT"[(v >> (2 * (ref_k - 1 - i))) & 3] for i in range(ref_k)) for v in val]
    centres = [t[4:39] for t in text]
    raw = np.zeros(c.total, dtype=np.uint32)
    raw[:] = c.records[:, c.sb]
    want_cnt = np.where((raw >= c.min_count) & (raw <= c.max_count), raw, 0).astype(np.uint32)
    assert np.array_equal(want_cnt, c.cnt)
    obf, octx, omap = ocapi.BF(bits), ocapi.BF(bits), ocapi.KMAP()
    for km in centres[0::3]:
        obf.add_key(km)
    for km in centres[1::7]:
        omap.add_key(km)
    for t in text[0::30]:
        octx.add_key(t)
    obf.switch_mode()
    octx.switch_mode()
    ocapi.kmc_scan_packed(octx, obf, omap, c.hi, c.lo, c.cnt, k, ref_k)
    with Context(k, ref_k, bits) as ctx:
        ctx.map_insert(rows_of(centres[1::7]))
        ctx.bf_insert(BF_ALT, rows_of(centres[0::3]))
        ctx.bf_finalize(BF_ALT)
        ctx.bf_insert(BF_CTX, rows_of(text[0::30]))
        ctx.bf_finalize(BF_CTX)
        _set(ctx, c)
        for first, n in c.runs:
            ctx.kmc_scan_records(c.records[first:first + n], first_record=first)
        counts = ctx.bf_export(BF_ALT)[3]
        assert np.array_equal(counts, obf.counts()) and counts.any()
        keys, vals = ctx.map_export()
        assert dict(zip(keys, (int(v) for v in vals))) == dict(omap.items()) and any(int(v) for v in vals)


def test_decode_across_the_host_piece_seam():
    """a run of 2^24 + 1 records of 2 bytes that starts at record 2 of the database: its second piece is the one last record, which
    must be decoded as record first_record + 2^24 of the table.  Measured on an MI355X: 0.27 s for the test, the case's numpy
    tables included."""
    lut, records, hi, lo, cnt = kc.piece_case()
    first, n = kc.PIECE_RUN
    assert n == kc.HOST_PIECE + 1 and first > 0 and first + n == len(lo)
    with Context(13, 13, 1 << 20) as ctx:
        ctx.kmc_set_lut(lut, 9, 1, 1, 2, 255, len(lo))
        ghi, glo, gcnt = ctx.kmc_decode_records(records[first:], first_record=first)
        assert (glo[-1], ghi[-1], gcnt[-1]) == (lo[-1], 0, cnt[-1])
        assert np.array_equal(glo, lo[first:]) and not ghi.any() and np.array_equal(gcnt, cnt[first:])
