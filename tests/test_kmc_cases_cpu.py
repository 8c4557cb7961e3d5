"""tests/kmc_cases.py proved without a GPU: every seam is named by a case; the checker's reading of each case's bytes (KmcDb.table():
a search of the prefix table) returns the items the bytes were written from, so case and checker agree by two routes; and every
claim a case's name makes -- which entry of its tile's window a record lies at, which entries are empty, where a bin ends, which
counts the bounds leave out -- holds on the case's own tables.  Nothing is skipped."""
import numpy as np
import pytest

import kmc_cases as kc
from oracle import kmc_db

U = np.uint64
IDS = kc.case_ids()


def as_db(c):
    """the case's tables as the checker's reader holds them (no files)"""
    db = object.__new__(kmc_db.KmcDb)
    db.k, db.lut_prefix_len, db.suffix_bytes, db.counter_size, db.min_count, db.max_count = c.k, c.p, c.sb, c.cb, c.min_count, c.max_count
    db.total, db.lut, db.records, db.rec = c.total, c.lut, c.records, c.sb + c.cb
    return db


def test_every_seam_is_named_by_a_case():
    table = {s: [n for n in IDS if s in kc.case(n).seams] for s in kc.SEAMS}
    assert all(table.values()), [s for s, v in table.items() if not v]
    named = {s for n in IDS for s in kc.case(n).seams}
    assert named <= set(kc.SEAMS), named - set(kc.SEAMS)


@pytest.mark.parametrize("name", IDS)
def test_the_listing_of_the_bytes_returns_the_items(name):
    c = kc.case(name)
    hi, lo, cnt = as_db(c).table()
    assert np.array_equal(hi, c.hi) and np.array_equal(lo, c.lo) and np.array_equal(cnt, c.cnt)
    # the table as mg_kmc_set_lut wants it, and the entry every record was filed under, by the search
    single = 1 << (2 * c.p)
    assert c.lut[0] == 0 and (np.diff(c.lut.astype(np.int64)) >= 0).all() and c.lut[-1] <= c.total and len(c.lut) % single == 0
    j = np.searchsorted(c.lut, np.arange(c.total, dtype=U), side="right") - 1
    assert np.array_equal(j, c.entry)
    assert c.k == c.p + 4 * c.sb <= 64 and c.p <= 10 and c.records.shape == (c.total, c.sb + c.cb)
    assert all(0 <= f and n >= 1 and f + n <= c.total for f, n in c.runs)


@pytest.mark.parametrize("name", IDS)
def test_case_holds_what_it_says(name):
    c = kc.case(name)
    cl = c.claims
    single = 1 << (2 * c.p)
    tiles = [t for run in c.runs for t in kc.tiles_of(c, run)]
    rel = lambda t: set((c.entry[t[0]:t[0] + t[1]] - t[2]).tolist())
    if "shape" in c.seams:
        assert "shift-%d" % (8 * c.sb) in c.seams and ((c.sb + c.cb) % 2 == 1) == ("odd-record-size" in c.seams)
        assert (c.hi != 0).any() == (c.k > 32) and (c.cnt == 0).any() and (c.cnt != 0).any()
    if "k-64" in c.seams:
        assert c.k == 64
    if "top-bits" in c.seams:
        assert int((c.hi >> U(56) == U(0xFF)).sum()) >= cl["top"] and c.p == 4 and (c.entry % single == single - 1).sum() >= cl["top"]
    if name == "counts-r3":
        assert (c.sb + c.cb) == 3 and {n for _, n in c.runs} >= {1, 1023, 1024, 1025, 2049} and {f for f, _ in c.runs} >= {0, 1, c.total - 1}
        assert (1000, 1024) in c.runs and all((n * 3) % 4 for n in (1, 1023, 1025, 2049))        # a last dword that is partly the tile's
    if cl.get("mid"):
        assert all(c.entry[f - 1] == c.entry[f] and c.lut[c.entry[f]] < f for f, _ in c.runs)
    if "j0" in cl:
        first = tiles[0]
        assert first[2] == cl["j0"] and rel(first) >= set(cl["offsets"]), sorted(rel(first))[:20]
        for e in cl.get("empty", ()):
            assert c.lut[cl["j0"] + e] == c.lut[cl["j0"] + e + 1]
        if "empty" in cl:                                       # the first record beyond the empty entries IS sh_lut[KMC_WIN]
            nxt = min(o for o in cl["offsets"] if o > max(cl["empty"]))
            g = int(c.lut[cl["j0"] + kc.KMC_WIN])
            assert c.entry[g] == cl["j0"] + nxt and nxt > kc.KMC_WIN and g < first[0] + first[1]
        if "window-edge" in c.seams:                            # entry j0 + 512 holds records: its first one equals sh_lut[KMC_WIN]
            g = int(c.lut[cl["j0"] + kc.KMC_WIN])
            assert c.entry[g] == cl["j0"] + kc.KMC_WIN and g < first[0] + first[1]
    if "beyond-window" in c.seams:
        assert any(max(rel(t)) > 4000 for t in tiles)             # several thousand entries beyond j0: the whole table is searched
    if cl.get("near_end"):
        assert all(t[2] + kc.KMC_WIN > len(c.lut) for t in tiles) and len(tiles) == 2 and tiles[1][2] != tiles[0][2]
        last = int(c.entry[-1])
        assert last < len(c.lut) - 1 and (c.lut[last + 1:] == c.total).all()                       # trailing empty prefixes
    if "drop" in cl:
        d = cl["drop"]
        assert c.entry[d - 1] // single == 0 and c.entry[d] // single == 1 and c.entry[d - 1] % single > c.entry[d] % single
        assert 0 < d < kc.KMC_TILE < c.total                      # inside the first tile
        if "beyond-window" in c.seams:
            assert c.entry[d] - c.entry[0] > kc.KMC_WIN
    if "empty_bin" in cl:
        b = cl["empty_bin"]
        assert len(set(c.lut[b * single:(b + 1) * single].tolist())) == 1 and not (c.entry // single == b).any() and len(c.lut) == 3 * single
        if b == 0:
            assert c.lut[single - 1] == 0 and c.entry[0] >= single
        if b == 2:
            assert (c.lut[2 * single:] == c.total).all()
    if "count-bounds" in c.seams:
        raw = c.records[:, c.sb].astype(np.int64)
        assert {max(c.min_count - 1, 0), c.min_count, 200, 201, 0} <= set(raw.tolist()) and c.max_count == 200
        assert np.array_equal(c.cnt, np.where((raw >= c.min_count) & (raw <= 200), raw, 0))
    if "count-u32" in c.seams:
        raw = c.records[:, c.sb:].copy().view("<u4").reshape(-1)
        assert c.cb == 4 and (raw == 0xFFFFFFFF).any()
        assert bool((c.cnt == 0xFFFFFFFF).any()) == cl["keeps_max"] and (c.cnt == 0xFFFFFFFE).any()
    if "scan" in c.seams:
        assert c.k == 43 and len(c.runs) == 2 and c.runs[1][0] == c.runs[0][1] and sum(n for _, n in c.runs) == c.total and len(c.lut) == 3 << 14


def test_the_piece_case_ends_one_record_into_the_second_piece():
    lut, records, hi, lo, cnt = kc.piece_case()
    first, run = kc.PIECE_RUN
    n = first + run
    assert run == kc.HOST_PIECE + 1 and first > 0
    prefix = lambda g: int(lo[g]) >> 8                          # the run's last record, and what a piece loop that dropped a term would look up
    assert len({prefix(n - 1), prefix(kc.HOST_PIECE), prefix(first), prefix(0)}) == 4
    assert records.shape == (n, 2) and len(lut) == 1 << 18 and lut[0] == 0 and (np.diff(lut.astype(np.int64)) >= 0).all() and lut[-1] <= n
    assert (np.diff(lo.astype(np.int64)) > 0).all() and int(lo[-1]) < 1 << 26
    for sl in (slice(0, 3000), slice(kc.HOST_PIECE - 1500, n)):    # the listing's search, on both sides of the seam
        g = np.arange(n, dtype=U)[sl]
        j = (np.searchsorted(lut, g, side="right") - 1).astype(U)
        assert np.array_equal((j << U(8)) | records[sl, 0].astype(U), lo[sl]) and np.array_equal(records[sl, 1].astype(np.uint32), cnt[sl])
    assert 2 <= cnt.min() and cnt.max() <= 255
