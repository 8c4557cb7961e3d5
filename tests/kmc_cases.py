"""Directed cases for the KMC record decode (kmc_decode_kernel of csrc/scan_kernels.h behind mg_kmc_set_lut, mg_kmc_decode_records
and the piece loop of mg_kmc_scan_records).  No GPU, no files and no product import here: tests/test_kmc_cases_cpu.py proves on any
machine that every case holds what its name says; tests/test_gpu_kmc_edges.py hands the same cases to the device.

A case is a list of (k-mer, count) items dealt to bins.  The prefix table and the raw record bytes are written from them by hand,
with the layout rules oracle/kmc_db.py states: per bin and prefix value the number of the first record that carries it, records
numbered through in file order, inside a bin ascending; a record is the suffix (big-endian, 4 symbols per byte) and the counter
(little-endian).  The EXPECTED ROWS ARE THE ITEMS THEMSELVES: hi / lo from the k-mer's 2k-bit value, the count or 0 where
[min_count, max_count] leaves it out -- never a search of the table.  Every item also records the table entry it was filed under
(bin * 4^p + prefix), so a claim such as "this record lies at entry j0 + 512 of its tile" is arithmetic on what the case made.

The kernel's geometry, restated (scan_kernels.h:1514-1560): a workgroup decodes a tile of KMC_TILE = 1,024 records; j0 is the entry of
the tile's first record; entries j0 .. j0 + 512 go to LDS and a record is searched there when its number is below entry j0 + 512's
(g < sh_lut[KMC_WIN]), in the whole table otherwise; entries beyond the table's end read as 2^64 - 1.

The HOST_PIECE seam of the host entries (2^24 records per staged piece) has a case of its own, made with numpy alone: piece_case()."""
import random
from collections import namedtuple

import numpy as np

KMC_TILE, KMC_WIN, HOST_PIECE = 1024, 512, 1 << 24
U = np.uint64
M64 = (1 << 64) - 1

Case = namedtuple("Case", "name seam p sb cb k min_count max_count lut records total hi lo cnt entry runs claims seams")
_CASES = {}


def kmer_value(kmer):
    v = 0
    for ch in kmer:
        v = (v << 2) | b"ACGT".index(ch)
    return v


def _add(name, seam, p, sb, cb, bins, min_count=2, max_count=255, runs=None, seams=(), **claims):
    """bins: per bin a list of (2k-bit value, count); sorted here, as a bin of the database is"""
    assert name not in _CASES, name
    k, single, rs = p + 4 * sb, 1 << (2 * p), sb + cb
    total = sum(len(b) for b in bins)
    lut = np.zeros(len(bins) * single, dtype=U)
    records = np.zeros((total, rs), dtype=np.uint8)
    hi, lo, cnt, entry = np.zeros(total, dtype=U), np.zeros(total, dtype=U), np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.int64)
    g = 0
    for b, items in enumerate(bins):
        items = sorted(items)
        assert len({v for v, _ in items}) == len(items), name
        per = np.zeros(single + 1, dtype=np.int64)
        for v, c in items:
            assert 0 <= v < 1 << (2 * k) and 0 <= c < 1 << (8 * cb)
            prefix = v >> (8 * sb)
            per[prefix + 1] += 1
            records[g, :sb] = np.frombuffer((v & ((1 << (8 * sb)) - 1)).to_bytes(sb, "big"), dtype=np.uint8)
            records[g, sb:] = np.frombuffer(c.to_bytes(cb, "little"), dtype=np.uint8)
            hi[g], lo[g] = v >> 64, v & M64
            cnt[g] = c if min_count <= c <= max_count else 0
            entry[g] = b * single + prefix
            g += 1
        lut[b * single:(b + 1) * single] = (g - len(items)) + np.cumsum(per)[:-1]
    _CASES[name] = Case(name, seam, p, sb, cb, k, min_count, max_count, lut, records, total, hi, lo, cnt, entry, tuple(runs or [(0, total)]), claims, tuple(seams))


def case_ids():
    return list(_CASES)


def case(name):
    return _CASES[name]


def tiles_of(c, run):
    """(first record, records, j0) of every tile of a run: j0 from the items' own entries"""
    first, n = run
    return [(first + t, min(KMC_TILE, n - t), int(c.entry[first + t])) for t in range(0, n, KMC_TILE)]


def _random_bins(rng, n, k, n_bins, counts):
    vals = set()
    while len(vals) < n:
        vals.add(rng.getrandbits(2 * k))
    bins = [[] for _ in range(n_bins)]
    for i, v in enumerate(sorted(vals)):
        bins[(v * 0x9E3779B97F4A7C15 >> 40) % n_bins].append((v, counts(i)))
    return bins


def _by_offsets(p, sb, base, offs, count=lambda i: 2 + i % 250):
    """one bin's items: record i has prefix base + offs[i]; suffixes ascend inside a prefix"""
    items, seen = [], {}
    for i, o in enumerate(offs):
        pre = base + o
        assert 0 <= pre < 1 << (2 * p)
        s = seen.get(pre, 0)
        seen[pre] = s + 1
        assert 10 * s + 3 < 1 << (8 * sb)
        items.append(((pre << (8 * sb)) | (10 * s + 3), count(i)))
    return items


def _build():
    rng = random.Random(20240)
    # -- record shapes
    for p, sb, cb, n in ((1, 1, 1, 500), (1, 1, 4, 500), (4, 15, 4, 2049), (8, 14, 1, 1500), (9, 1, 1, 1500), (3, 7, 1, 1500), (3, 8, 1, 1500), (3, 9, 1, 1500)):
        big = (1 << (8 * cb)) - 1
        _add("shape-p%d-s%d-c%d" % (p, sb, cb), "records of %d + %d bytes, k = %d: 8 * suffix_bytes = %d" % (sb, cb, p + 4 * sb, 8 * sb), p, sb, cb,
             _random_bins(rng, n, p + 4 * sb, 2, lambda i: (1 + i % 300) if cb > 1 else (1 + i % 255)), max_count=min(big, 1000), runs=[(0, n), (n // 3 + 5, n - n // 3 - 5)],
             seams=["shape", "shift-%d" % (8 * sb)] + (["odd-record-size"] if (sb + cb) % 2 else []) + (["k-64"] if p + 4 * sb == 64 else []))
    k = 64
    top = [((0xFF << 120) | rng.getrandbits(120), 5 + i) for i in range(40)]
    _add("k64-prefix-TTTT", "k = 64, the prefix TTTT: the top byte of hi is set from the table entry alone", 4, 15, 1, [top + [(rng.getrandbits(128), 9) for _ in range(300)]],
         seams=["k-64", "top-bits"], top=40)
    # -- record counts and first records, at a record size of 3
    db = _random_bins(rng, 4000, 11, 1, lambda i: 2 + i % 200)
    runs = [(0, 1), (0, 1023), (0, 1024), (0, 1025), (0, 2049), (1, 2049), (3999, 1), (1000, 1024), (0, 4000)]
    _add("counts-r3", "runs of 1, 1,023, 1,024, 1,025 and 2,049 records of 3 bytes (the dword tail of the staged bytes); first_record 0, 1, total - 1; one tile from record 1,000",
         3, 2, 1, db, runs=runs, seams=["n-1", "n-1023", "n-1024", "n-1025", "n-2049", "first-1", "first-last", "tile-at-1000", "odd-record-size"])
    _add("mid-prefix", "a run whose first record shares its prefix with the record before it", 3, 2, 1, _random_bins(rng, 4000, 11, 1, lambda i: 2 + i % 200),
         runs=[(1501, 1025), (2000, 2000)], seams=["first-mid-prefix"], mid=True)
    # -- the window of 512 entries
    offs = [0] * 200 + [510] + [511] * 2 + [512] * 2 + [513] + [3000] * 300 + [9000] * 528 + [9001 + i for i in range(600)] + [16283] * 5
    _add("window-edge", "a tile over thousands of entries, records at entries j0 + 510 .. j0 + 513 and far beyond", 7, 2, 1, [_by_offsets(7, 2, 100, offs)],
         runs=[(0, len(offs)), (1024, len(offs) - 1024), (600, 1024)], seams=["window-edge", "beyond-window"], j0=100, offsets=[0, 510, 511, 512, 513, 3000, 9000])
    offs = [0] * 300 + [510] * 2 + [514] * 3 + [515] + [600] * 718 + [601] * 50
    _add("window-equal-entries", "entries j0 + 511 .. j0 + 513 are empty and equal entry j0 + 514: its first record equals sh_lut[KMC_WIN]", 7, 2, 1, [_by_offsets(7, 2, 2000, offs)],
         seams=["window-equal"], j0=2000, offsets=[0, 510, 514, 515], empty=[511, 512, 513])
    offs = [0] * 300 + [511] * 2 + [513] * 2 + [700] * 720 + [701] * 50
    _add("window-empty-512", "entry j0 + 512 is empty and equals entry j0 + 513", 7, 2, 1, [_by_offsets(7, 2, 2000, offs)], seams=["window-equal"], j0=2000, offsets=[0, 511, 513],
         empty=[512])
    offs = [0] * 400 + [40] * 400 + [90] * 300 + [94] * 100
    _add("table-end", "j0 within 512 entries of the table's end; trailing empty prefixes whose entries equal the total; the database's last record", 7, 2, 1,
         [_by_offsets(7, 2, (1 << 14) - 100, offs)], seams=["table-end", "trailing-empty", "last-record"], near_end=True)
    # -- bins
    hi_items = lambda n, p, sb: _by_offsets(p, sb, (1 << (2 * p)) - 56, [i * 56 // n for i in range(n)])
    lo_items = lambda n, p, sb, base=0: _by_offsets(p, sb, base, [i * 50 // n for i in range(n)], count=lambda i: 3 + i % 100)
    _add("bin-boundary-p4", "a tile across a bin boundary: the prefix drops from high to low", 4, 2, 1, [hi_items(700, 4, 2), lo_items(700, 4, 2), lo_items(100, 4, 2, 100)],
         seams=["bin-boundary"], drop=700)
    _add("bin-boundary-p7", "the same, the next bin's entries more than 512 beyond j0", 7, 2, 1, [hi_items(700, 7, 2), lo_items(700, 7, 2, 5000)], seams=["bin-boundary", "beyond-window"],
         drop=700)
    _add("bin-empty-first", "an empty first bin: record 0 is filed in the second", 4, 2, 1, [[], lo_items(600, 4, 2, 20), hi_items(300, 4, 2)], seams=["empty-first-bin"], empty_bin=0)
    _add("bin-empty-middle", "an empty middle bin", 4, 2, 1, [hi_items(600, 4, 2), [], lo_items(300, 4, 2, 20)], seams=["empty-middle-bin"], empty_bin=1)
    _add("bin-empty-last", "an empty last bin: its entries equal the total", 4, 2, 1, [hi_items(600, 4, 2), lo_items(300, 4, 2, 20), []], seams=["empty-last-bin", "trailing-empty"],
         empty_bin=2)
    # -- counts
    cyc = [2, 3, 200, 201, 0, 7, 255]
    for mn in (0, 1, 3):
        _add("count-bounds-min%d" % mn, "counts min - 1, min, max, max + 1 and 0 with min_count %d, max_count 200" % mn, 3, 2, 1,
             _random_bins(rng, 1100, 11, 2, lambda i: (cyc + [mn, max(mn - 1, 0), 1])[i % 10]), min_count=mn, max_count=200, seams=["count-bounds", "min-%d" % mn])
    big4 = [(1 << 32) - 1, (1 << 32) - 2, 1, 0, 70000, 1 << 31]
    for tag, mx in (("2^32-1", (1 << 32) - 1), ("2^40", 1 << 40), ("2^32-2", (1 << 32) - 2)):
        _add("count-u32-max-" + tag, "4-byte counters holding 2^32 - 1, max_count " + tag, 3, 2, 4, _random_bins(rng, 1100, 11, 2, lambda i: big4[i % 6]), min_count=1, max_count=mx,
             seams=["count-u32"], keeps_max=mx >= (1 << 32) - 1)
    # -- the second table of the replacement test, and the scan's
    _add("first-table-k11", "k = 11 as 7 + 4 * 1: a table of 2 x 4^7 entries, records of 2 bytes (the table that count-u32-max-2^40, 3 + 4 * 2, replaces)", 7, 1, 1,
         _random_bins(rng, 2500, 11, 2, lambda i: 1 + i % 255), seams=["replace"])
    _add("scan-43", "43-mers for mg_kmc_scan_records: two runs whose first records differ", 7, 9, 1, _random_bins(rng, 3000, 43, 3, lambda i: 1 + i % 255), seams=["scan"],
         runs=[(0, 1700), (1700, 1300)])


_build()

SEAMS = ["shape", "shift-8", "shift-56", "shift-64", "shift-72", "shift-112", "shift-120", "odd-record-size", "k-64", "top-bits", "n-1", "n-1023", "n-1024", "n-1025", "n-2049", "first-1",
         "first-last", "first-mid-prefix", "tile-at-1000", "window-edge", "window-equal", "beyond-window", "table-end", "trailing-empty", "last-record", "bin-boundary", "empty-first-bin",
         "empty-middle-bin", "empty-last-bin", "count-bounds", "min-0", "min-1", "min-3", "count-u32", "replace", "scan"]


PIECE_RUN = (100, HOST_PIECE + 1)                                      # (first record, records) of the run that crosses the seam


def piece_case():
    """the HOST_PIECE seam: a database of 2^24 + 101 records of 2 bytes (p = 9, one suffix byte, k = 13), distinct ascending values,
    one bin.  The run PIECE_RUN of 2^24 + 1 records starts at record 100: its second piece is one record, which must be decoded as
    record first_record + 2^24 -- under another prefix than record 2^24 and record 100, which a loop that dropped either term
    would look up.  -> (lut, records, hi, lo, cnt), numpy only"""
    n = sum(PIECE_RUN)
    v = np.arange(n, dtype=U) * U(3) + U(1)                                # below 4^13
    cnt = (np.arange(n, dtype=np.uint32) % np.uint32(250) + np.uint32(2)).astype(np.uint32)
    records = np.empty((n, 2), dtype=np.uint8)
    records[:, 0] = (v & U(255)).astype(np.uint8)
    records[:, 1] = cnt.astype(np.uint8)
    lut = np.searchsorted(v >> U(8), np.arange(1 << 18, dtype=U), side="left").astype(U)
    return lut, records, np.zeros(n, dtype=U), v, cnt
