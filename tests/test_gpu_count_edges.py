"""The four cell counters behind `call --cohort` -- mg_pack_dosage, mg_pair_counts, mg_sample_counts, mg_site_counts and
mg_site_geno_counts -- on the directed cases of tests/count_cases.py: a cell on every seam of chunk, run, tile, carry, storing lane,
step and round of bins; tests/test_count_cases_cpu.py proves that each case holds what it claims and that its expectation is the
restatements'.  Every case goes through the host form and the device form (into buffers with guard words on both sides), fresh and as
two or more accumulating calls cut at the case's seam -- the words, the records, or for the site kernels the planes.  Every comparison
is exact equality of integers."""
import ctypes as C

import numpy as np
import pytest
import torch

import count_cases as cc
from malva_amd import Context
from malva_amd.capi import SAMPLE_SLOTS
from test_sample_stats_cpu import SLOT_NAMES

pytestmark = pytest.mark.gpu
PAD = 64
GUARD32, GUARD64 = 0xAAAAAAAA, 0xAAAAAAAAAAAAAAAA
POISON64 = np.uint64(0xDEADBEEFDEADBEEF)
COUNTED = len(SLOT_NAMES)
RUN = {kind: [c for c in cc.cases() if c.kind == kind] for kind in ("pair", "pack", "sample", "site")}
of_kind = lambda kind: pytest.mark.parametrize("case", RUN[kind], ids=lambda c: c.name)
v = C.c_void_p


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def _dev(a):
    """a host array on the device, as bytes (None stays None)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a if a.size else np.zeros(1, a.dtype)).reshape(-1).view(np.uint8)).to(torch.device("cuda", 0))


def _ptr(t):
    return v(None if t is None else t.data_ptr())


class Guarded:
    """a device buffer of `fill` (a number or an array) with PAD guard words on both sides"""

    def __init__(self, fill, size, dtype):
        self.size, self.dtype = size, np.dtype(dtype)
        self.guard = GUARD32 if self.dtype.itemsize == 4 else GUARD64
        h = np.full(size + 2 * PAD, self.guard, dtype=dtype)
        h[PAD:PAD + size] = fill
        self.t = _dev(h)

    def ptr(self):
        return v(self.t.data_ptr() + PAD * self.dtype.itemsize)

    def read(self, what):
        h = self.t.cpu().numpy().view(self.dtype)
        assert (h[:PAD] == self.guard).all(), "%s: words in front of the output were written" % what
        assert (h[PAD + self.size:] == self.guard).all(), "%s: words behind the output were written" % what
        return h[PAD:PAD + self.size].copy()


# ---- pairs, counting ----------------------------------------------------------------------------------------------------------------

def _same_pairs(got, want, what):
    if not np.array_equal(got, want):
        i, j, da, db = (int(x[0]) for x in np.nonzero(got != want))
        raise AssertionError("%s: first difference at (i, j, da, db) = (%d, %d, %d, %d): %d, expected %d" % (what, i, j, da, db, int(got[i, j, da, db]), int(want[i, j, da, db])))


def _pairs_device(ctx, case, parts, start, accumulate):
    """parts: (A, B) operands counted one after the other into one guarded table that starts as `start`"""
    table = Guarded(start.reshape(-1), start.size, np.uint64)
    for k, (a, b) in enumerate(parts):
        da, db = _dev(a), _dev(b)
        torch.cuda.synchronize()
        ctx._ck(ctx._L.mg_pair_counts_device(ctx.h, a.shape[2], _ptr(da), case.n_a, _ptr(db), case.n_b, int(accumulate or k > 0), table.ptr()))
        ctx.synchronize()
    return table.read(case.name).reshape(start.shape)


@of_kind("pair")
def test_pair_case(ctx, case):
    a, b = case.planes()
    want = case.expected()
    cut = lambda p, lo, hi: None if p is None else np.ascontiguousarray(p[:, :, lo:hi])
    parts = [(cut(a, 0, case.cut), cut(b, 0, case.cut)), (cut(a, case.cut, case.n_words), cut(b, case.cut, case.n_words))]
    start = case.start_table()
    summed = start + want                                                          # (uint64: wraps as the table does)
    # the host form: fresh over garbage, then two accumulating calls cut at the case's word on top of its start table
    fresh = ctx.pair_counts(a, b, counts=np.full(want.shape, POISON64, dtype=np.uint64), overwrite=True)
    _same_pairs(fresh, want, case.name + ", host form")
    table = start.copy()
    for pa, pb in parts:
        ctx.pair_counts(pa, pb, counts=table)
    _same_pairs(table, summed, case.name + ", host form, two accumulating calls")
    # the device form
    _same_pairs(_pairs_device(ctx, case, [(a, b)], np.full(want.shape, POISON64, dtype=np.uint64), False), want, case.name + ", device form")
    _same_pairs(_pairs_device(ctx, case, parts, start, True), summed, case.name + ", device form, two accumulating calls")
    if case.start is not None:                                                     # one accumulating call over all the words
        _same_pairs(_pairs_device(ctx, case, [(a, b)], start, True), summed, case.name + ", device form, one accumulating call")


def test_pack_feeds_count_on_a_trip_shape(ctx):
    """2 planes x 65,537 words, one tile, runs of two chunks: the cells go through mg_pack_dosage_device and from there through
    mg_pair_counts_device without leaving the device, B NULL and B given"""
    e = cc.pack_to_count()
    n, W = e.n, e.n_words
    d1, d2, dv = _dev(e.g1), _dev(e.g2), _dev(e.vao())
    planes = Guarded(GUARD64 ^ 0xFFFF, 2 * 3 * W, np.uint64)
    torch.cuda.synchronize()
    ctx._ck(ctx._L.mg_pack_dosage_device(ctx.h, n, 2, 0, _ptr(d1), _ptr(d2), None, 0, 0, _ptr(dv), planes.ptr()))
    want = e.expected()
    for b_given in (False, True):
        table = Guarded(int(POISON64), want.size, np.uint64)
        torch.cuda.synchronize()
        ctx._ck(ctx._L.mg_pair_counts_device(ctx.h, W, planes.ptr(), 2, planes.ptr() if b_given else None, 2, 0, table.ptr()))
        ctx.synchronize()
        _same_pairs(table.read("counts").reshape(want.shape), want, "pack feeds count, B %s" % ("given" if b_given else "NULL"))
    packed = planes.read("planes").reshape(2, 3, W)
    assert not (packed[:, :, W - 1] >> np.uint64(1)).any(), "the last word holds one record: bits at and beyond n_vars are set"
    for plane, d in enumerate(e.directed[n - 1]):
        assert [int(x) for x in packed[plane, :, W - 1]] == [int(k == d) for k in range(3)]


# ---- pairs, packing ----------------------------------------------------------------------------------------------------------------

@of_kind("pack")
def test_pack_case(ctx, case):
    want = case.expected()
    g2 = None if case.haploid else case.g2
    masked = case.min_gq is not None
    got = ctx.pack_dosage(case.g1, g2, case.gq if masked else None, case.haploid, case.vao(), min_gq=case.min_gq, out=np.full(want.shape, cc.ONES, dtype=np.uint64))
    d1, d2, dq, dv = _dev(case.g1), _dev(g2), _dev(case.gq if masked else None), _dev(case.vao())
    out = Guarded(GUARD64 ^ 0xFFFF, want.size, np.uint64)
    torch.cuda.synchronize()
    ctx._ck(ctx._L.mg_pack_dosage_device(ctx.h, case.n, case.planes, int(case.haploid), _ptr(d1), _ptr(d2), _ptr(dq), int(masked), int(case.min_gq or 0), _ptr(dv), out.ptr()))
    ctx.synchronize()
    for form, g in (("host", got), ("device", out.read(case.name).reshape(want.shape))):
        if not np.array_equal(g, want):
            p, d, w = (int(x[0]) for x in np.nonzero(g != want))
            raise AssertionError("%s, %s form: first difference at (plane, dosage, word) = (%d, %d, %d): %#x, expected %#x" % (case.name, form, p, d, w, int(g[p, d, w]), int(want[p, d, w])))


# ---- the sample table ---------------------------------------------------------------------------------------------------------------

def _same_table(got, want, what):
    if not np.array_equal(got, want):
        p, k = (int(x[0]) for x in np.nonzero(got != want))
        raise AssertionError("%s: first difference at (plane, slot) = (%d, %s): %d, expected %d" % (what, p, SLOT_NAMES[k] if k < COUNTED else k, int(got[p, k]), int(want[p, k])))


def _sample_parts(case, cuts):
    """the case's arrays cut at the records `cuts`: (g1, g2, gq, vao, status, cov, classes) per part"""
    vao, cls = case.vao(), case.allele_class()
    parts = []
    for lo, hi in zip(cuts, cuts[1:]):
        a0, a1 = int(vao[lo]), int(vao[hi])
        s = lambda x: None if x is None else np.ascontiguousarray(x[:, lo:hi])
        parts.append((s(case.g1), s(case.g2), s(case.gq), (vao[lo:hi + 1] - vao[lo]).astype(np.uint32), s(case.status),
                      None if case.cov is None else np.ascontiguousarray(case.cov[:, a0:a1]), None if cls is None else np.ascontiguousarray(cls[a0:a1])))
    return parts


def _sample_device(ctx, case, parts, start, accumulate):
    table = Guarded(start.reshape(-1), start.size, np.uint64)
    masked = case.min_gq is not None
    for k, part in enumerate(parts):
        g1, g2, gq, vao, status, cov, cls = part
        d = [_dev(x) for x in part]
        torch.cuda.synchronize()
        ctx._ck(ctx._L.mg_sample_counts_device(ctx.h, g1.shape[1], case.planes, 0, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), int(masked), int(case.min_gq or 0), _ptr(d[4]),
                                               _ptr(d[5]), _ptr(d[3]), _ptr(d[6]), int(accumulate or k > 0), table.ptr()))
        ctx.synchronize()
    return table.read(case.name).reshape(start.shape)


@of_kind("sample")
def test_sample_case(ctx, case):
    want = case.expected()
    whole = _sample_parts(case, (0, case.n))
    halves = _sample_parts(case, (0, case.cut, case.n))
    start = case.start_table()
    summed = start + want                                                          # (uint64: wraps as the table does; the reserved slots keep the start)
    poisoned = lambda: np.full((case.planes, SAMPLE_SLOTS), POISON64, dtype=np.uint64)
    call = lambda part, **kw: ctx.sample_counts(part[0], part[1], part[2], False, part[3], part[4], part[5], part[6], min_gq=case.min_gq, **kw)
    _same_table(call(whole[0], counts=poisoned(), overwrite=True), want, case.name + ", host form")
    table = start.copy()
    for part in halves:
        call(part, counts=table)
    _same_table(table, summed, case.name + ", host form, two accumulating calls")
    _same_table(_sample_device(ctx, case, whole, poisoned(), False), want, case.name + ", device form")
    _same_table(_sample_device(ctx, case, halves, start, True), summed, case.name + ", device form, two accumulating calls")
    if case.start is not None:
        _same_table(_sample_device(ctx, case, whole, start, True), summed, case.name + ", device form, one accumulating call")


# ---- site tags and site genotype counts -----------------------------------------------------------------------------------------------

def _same_counts(got, want, vao, what):
    """got / want: tuples of arrays per record or per slot"""
    for g, w, name in zip(got, want, what[1]):
        if not np.array_equal(g, w):
            k = int(np.nonzero(g != w)[0][0])
            where = "record %d" % k if g.size == vao.size - 1 and name in ("ns", "n") else "record %d, allele %d" % (int(np.searchsorted(vao, k, side="right")) - 1,
                                                                                                                      k - int(vao[int(np.searchsorted(vao, k, side="right")) - 1]))
            raise AssertionError("%s: %s first differs at %s: %d, expected %d" % (what[0], name, where, int(g[k]), int(w[k])))


def _site_device(ctx, case, entry, groups, start, sizes, accumulate):
    """entry: 'tags' or 'geno'; the plane groups one call after the other into guarded outputs that start as `start`"""
    vao = case.vao()
    dv = _dev(vao)
    outs = [Guarded(s, size, np.uint32) for s, size in zip(start, sizes)]
    for k, (lo, hi) in enumerate(zip(groups, groups[1:])):
        d1, d2, dq = _dev(case.g1[lo:hi]), _dev(case.g2[lo:hi]), _dev(case.gq[lo:hi])
        torch.cuda.synchronize()
        f = ctx._L.mg_site_counts_device if entry == "tags" else ctx._L.mg_site_geno_counts_device
        ctx._ck(f(ctx.h, case.n, hi - lo, 0, _ptr(d1), _ptr(d2), _ptr(dq), 1, case.min_gq, _ptr(dv), int(accumulate or k > 0), *(o.ptr() for o in outs)))
        ctx.synchronize()
    return tuple(o.read(case.name + ", " + entry) for o in outs)


@of_kind("site")
def test_site_case(ctx, case):
    vao = case.vao()
    slots = int(vao[-1])
    tags, geno = case.expected()
    whole = (0, case.planes)
    for entry, want, sizes, names in (("tags", tags, (slots, case.n), ("ac", "ns")), ("geno", geno, (case.n, slots, slots), ("n", "het", "hom"))):
        host = ctx.site_counts if entry == "tags" else ctx.site_geno_counts
        if case.planes <= 64:                                                      # fresh: the host form into new arrays, the device form over poison
            got = host(case.g1, case.g2, case.gq, False, vao, min_gq=case.min_gq)
            _same_counts(got, want, vao, (case.name + ", host form", names))
            got = _site_device(ctx, case, entry, whole, [0xDEADBEEF] * len(sizes), sizes, False)
            _same_counts(got, want, vao, (case.name + ", device form", names))
        # the plane groups one accumulating call after the other, on top of slots that hold 1,000
        summed = tuple(w + np.uint32(1000) for w in want)
        acc = [np.full(size, 1000, dtype=np.uint32) for size in sizes]
        for lo, hi in zip(case.groups, case.groups[1:]):
            if entry == "tags":
                host(case.g1[lo:hi], case.g2[lo:hi], case.gq[lo:hi], False, vao, min_gq=case.min_gq, ac=acc[0], ns=acc[1])
            else:
                host(case.g1[lo:hi], case.g2[lo:hi], case.gq[lo:hi], False, vao, min_gq=case.min_gq, n=acc[0], het=acc[1], hom=acc[2])
        _same_counts(acc, summed, vao, (case.name + ", host form, accumulating over the plane groups", names))
        got = _site_device(ctx, case, entry, case.groups, [1000] * len(sizes), sizes, True)
        _same_counts(got, summed, vao, (case.name + ", device form, accumulating over the plane groups", names))
