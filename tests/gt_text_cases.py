"""Sample columns that drive the GT text decoder (csrc/gt_text_kernels.h: gt_decode_kernel -> gt_compact_kernel) onto every seam
of its tab scan, its persistent loops and its compaction, and what oracle/model.py's VCFReader reads in them.  No GPU and no
product import here: tests/test_gt_text_cases_cpu.py checks on any machine that every case holds, byte for byte, what it claims;
tests/test_gpu_gt_text_edges.py hands the same bytes to the device.

A case is a small VCF: a FORMAT string and the column strings per record, the header's sample count, an optional keep mask, the
modes (diploid, haploid) it runs in, and its claims.  Claims speak of the bytes `_spans` returns, never of what a decoder makes
of them:
    ("records", n)               the case has n records
    ("span_len", r, n)           record r's sample columns are n bytes
    ("tab", r, o)                byte o of record r's span is a tab (o < 0 counts from the end)
    ("no_tab", r, a, b)          bytes [a, b) of record r's span hold no tab
    ("cols", r, n)               record r has n sample columns (fewer than the header: a short record; 0: none at all)
    ("gt_index", r, i)           GT is FORMAT key i of record r
    ("ploidy", r, p)             the longest GT among record r's kept columns has p values
    ("zero_words", p, u)         the kept columns of the batch spell p times "0|0" and u times "0/0" (and no other form of either)
    ("odd_kept", r, [s...])      the kept samples of record r whose column differs from the record's commonest one
    ("text_off", r, o)           record r's span starts at least o bytes into the file
    ("select", [r...])           the batch handed to the decoder: these records in this order (default: all, file order)
    ("max_only", [r...])         records the model is not asked about (allele numbers past 32,767): only max_allele == 32767 holds
    ("default", w)               the diploid batch's default word (haploid: always 1 << 14)
GT forms are those a VCF may hold: digits, ".", empty, "/" and "|", any ploidy, leading zeros, large numbers."""
import functools
import os
import zlib
from collections import Counter, namedtuple

import numpy as np

from oracle import model

PIECE, WAVE_BYTES, TILE = 16, 1024, 4096     # bytes of a lane, a wave and a tile of the tab scan
COMPACT_TILE = 256                           # samples per pass of gt_compact_kernel (and of the decode kernel's fill loop)
DECODE_GRID, COMPACT_GRID = 1024, 2048       # workgroups of the two persistent loops
MAX_GT_INDEX = 1000
PHASED0 = 1 << 14

Case = namedtuple("Case", "name fmts records n_columns keep modes claims pad_header")
Built = namedtuple("Built", "raw off ln gi n_columns keep n_keep want masks maxes select")


# ---- the VCF of a case, its spans, the model's reading (shared with tests/test_gpu_gt_text.py) ------------------------------
def _write(path, records, n_samples, fmt_of=lambda i: "GT", pad=False, pad_header=0):
    """pad: records with fewer sample columns than the header are completed with "." -- what the product reads them as;
    the oracle's reader (like htslib) has no opinion on such a record, so it is given the completed one.
    pad_header: bytes of a ## comment line in front of everything (moves the records that far into the text)"""
    if pad:
        records = [(list(c) if c is not None else []) + ["."] * (n_samples - (len(c) if c is not None else 0)) for c in records]
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n##INFO=<ID=AF,Number=A,Type=Float,Description=\"af\">\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"g\">\n")
        if pad_header:
            fh.write("##filler=" + "x" * pad_header + "\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("S%d" % i for i in range(n_samples)) + "\n")
        for i, cells in enumerate(records):
            fh.write("1\t%d\t.\tA\tC,G,T\t.\t.\tAF=0.1,0.1,0.1\t%s\t%s\n" % (100 + 40 * i, fmt_of(i), "\t".join(cells)) if cells is not None else
                     "1\t%d\t.\tA\tC,G,T\t.\t.\tAF=0.1,0.1,0.1\t%s\n" % (100 + 40 * i, fmt_of(i)))


def _spans(path):
    """what the host side of the decode does: per record line, where its sample columns start and end, and where GT sits in FORMAT"""
    raw = open(path, "rb").read()
    off, ln, gi = [], [], []
    at = 0
    for line in raw.split(b"\n"):
        if line and not line.startswith(b"#"):
            cols = line.split(b"\t", 9)
            gi.append(cols[8].split(b":").index(b"GT"))
            if len(cols) > 9:
                off.append(at + len(line) - len(cols[9]))
                ln.append(len(cols[9]))
            else:
                off.append(at + len(line))
                ln.append(0)
        at += len(line) + 1
    return raw, np.array(off, np.uint64), np.array(ln, np.uint32), np.array(gi, np.int32)


def _expected(path, samples_file, haploid):
    rd = model.VCFReader(path, samples_file or "-")
    words, masks, mx = [], [], []
    for v in rd.records():
        w = []
        m = 0
        big = 0
        for (a1, a2), ph in zip(v.genotypes, v.phasing):
            w.append((a1 & 127) | (1 << 14) if haploid else (a1 & 127) | (a2 & 127) << 7 | int(ph) << 14)
            m |= 1 << (a1 & 63)
            if not haploid:
                m |= 1 << (a2 & 63)
            big = max(big, a1, a2)
        words.append(np.array(w, np.uint16))
        masks.append(m)
        mx.append(big)
    return words, masks, mx


def _dense(n_keep, dflt, sp_off, ss, sg):
    out = []
    for r in range(len(sp_off) - 1):
        w = np.full(n_keep, dflt, np.uint16)
        e0, e1 = int(sp_off[r]), int(sp_off[r + 1])
        assert np.all(np.diff(ss[e0:e1].astype(np.int64)) > 0)          # ascending samples inside a record
        assert np.all(sg[e0:e1] != dflt)                                 # only the words that differ from the default
        w[ss[e0:e1]] = sg[e0:e1]
        out.append(w)
    return out


def default_word(words, haploid):
    """the batch default as mg_decode_gt_text chooses it, from the model's words: 0/0 only where it strictly outnumbers 0|0"""
    p0 = sum(int((w == PHASED0).sum()) for w in words)
    u0 = sum(int((w == 0).sum()) for w in words)
    return PHASED0 if haploid or u0 <= p0 else 0


def build(case, directory, haploid):
    """write the case under `directory` -> Built: the decoder's arguments and the model's answer for the selected records"""
    path = os.path.join(directory, "case.vcf")
    fmt_of = lambda i: case.fmts[i]
    _write(path, case.records, case.n_columns, fmt_of, pad_header=case.pad_header)
    _write(path + ".padded", case.records, case.n_columns, fmt_of, pad=True, pad_header=case.pad_header)
    samples_file = None
    n_keep = case.n_columns
    if case.keep is not None:
        samples_file = os.path.join(directory, "keep.txt")
        with open(samples_file, "w") as fh:
            fh.write("".join("S%d\n" % i for i in np.flatnonzero(case.keep)))
        n_keep = int(np.count_nonzero(case.keep))
    want, masks, maxes = _expected(path + ".padded", samples_file, haploid)
    raw, off, ln, gi = _spans(path)
    assert len(want) == len(off) == len(case.records)
    select = claim(case, "select")
    sel = list(range(len(off))) if select is None else list(select[0])
    idx = np.array(sel, dtype=np.int64)
    return Built(raw, off[idx], ln[idx], gi[idx], case.n_columns, case.keep, n_keep, [want[r] for r in sel], [masks[r] & ((1 << 64) - 1) for r in sel],
                 [maxes[r] for r in sel], sel)


def claim(case, kind):
    """the arguments of the case's only claim of this kind, or None"""
    got = [c[1:] for c in case.claims if c[0] == kind]
    assert len(got) <= 1
    return got[0] if got else None


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _case(name, records, n_columns, claims, fmts="GT", keep=None, modes=(False, True), pad_header=0):
    fmts = [fmts] * len(records) if isinstance(fmts, str) else list(fmts)
    assert len(fmts) == len(records)
    if keep is not None:
        keep = np.asarray(keep, dtype=np.uint8)
        assert keep.shape == (n_columns,)
    return Case(name, fmts, records, n_columns, keep, tuple(modes), [("records", len(records))] + list(claims), pad_header)


# ---- columns of a wanted length, tabs at wanted offsets ------------------------------------------------------------------
_GT3 = ("0|1", "1|0", "2/1", "1|2", "3|0", "0/3", "1|1")


def column(length, c, behind=False):
    """a column of exactly `length` bytes for FORMAT GT:XX (behind: XX:GT), its GT depending on the column number c"""
    if length < 4 or (behind and length < 5):
        if behind:      # XX:GT: a column too short for both stops short of GT, or holds a one-byte filler
            return ["", "x", "x:", "x:%d" % (c % 4), "x:%d%d" % (1 + c % 2, c % 10)][length]
        return ["", "%d" % (c % 4), "%d%d" % (1 + c % 2, c % 10), _GT3[c % 7]][length]
    return "x" * (length - 4) + ":" + _GT3[c % 7] if behind else _GT3[c % 7] + ":" + "x" * (length - 4)


def cells_with_tabs(tabs, length, behind=False):
    """the columns of a span of `length` bytes whose tabs sit exactly at the (ascending) offsets `tabs`"""
    tabs = list(tabs)
    assert tabs == sorted(set(tabs)) and (not tabs or (tabs[0] >= 0 and tabs[-1] < length))
    edges = [-1] + tabs + [length]
    return [column(b - a - 1, c, behind) for c, (a, b) in enumerate(zip(edges, edges[1:]))]


def _tab_claims(r, tabs, length):
    out = [("span_len", r, length), ("cols", r, len(tabs) + 1)] + [("tab", r, t) for t in tabs]
    edges = [-1] + list(tabs) + [length]
    return out + [("no_tab", r, a + 1, b) for a, b in zip(edges, edges[1:]) if b > a + 1]


# ---- A: span geometry -------------------------------------------------------------------------------------------------------
SPAN_LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 12289)


def _a_span_lengths(name, behind):
    recs, claims = [], []
    for r, L in enumerate(SPAN_LENGTHS):
        tabs = [] if L < 15 else [L // 4, L // 2, 3 * L // 4]           # four columns, or a short record of one
        recs.append(cells_with_tabs(tabs, L, behind))
        claims += _tab_claims(r, tabs, L)
    return _case(name, recs, 4, claims, fmts="XX:GT" if behind else "GT:XX")


def _a_seam(name, where, behind):
    """a tab as the last (where = -1) or the first (0) byte of a piece of 16, a wave's 1,024, a tile's 4,096, and of the third tile"""
    recs, claims = [], []
    for r, seam in enumerate((PIECE, 3 * PIECE, WAVE_BYTES, 3 * WAVE_BYTES, TILE, 2 * TILE)):
        t = seam + where
        tabs = [3, 9, t, t + 9, t + 23]                                  # (no tab on the other side of the seam)
        L = t + 30
        recs.append(cells_with_tabs(tabs, L, behind))
        claims += _tab_claims(r, tabs, L)
        assert t % PIECE == (PIECE - 1 if where else 0) and (seam < WAVE_BYTES or t % WAVE_BYTES == (WAVE_BYTES - 1 if where else 0))
    return _case(name, recs, 6, claims, fmts="XX:GT" if behind else "GT:XX")


def _a_sixteen_tabs(name):
    recs, claims = [], []
    for r, base in enumerate((0, PIECE, WAVE_BYTES - PIECE, WAVE_BYTES, TILE - PIECE, TILE, 2 * TILE + 5 * PIECE)):
        tabs = ([5] if base >= PIECE else []) + list(range(base, base + PIECE)) + [base + 30]
        if base < PIECE:
            tabs.append(base + 40)                                       # every record: 19 columns
        L = tabs[-1] + 8
        recs.append(cells_with_tabs(tabs, L))
        claims += _tab_claims(r, tabs, L)
        assert base % PIECE == 0 and len(tabs) == 18
    return _case(name, recs, 19, claims, fmts="GT:XX")


def _a_tile_without_tab(name):
    recs, fmts, claims = [], [], []
    for r, (behind, first) in enumerate(((False, True), (True, True), (False, False), (True, False))):
        long_col = "x" * 5000 + ":1|2" if behind else "2|1:" + "x" * 5000         # GT behind 5,000 bytes of filler / in front of them
        if not first:
            long_col = "x" * 9000 + ":3|1" if behind else "1|3:" + "x" * 9000
        short = ["x:0|1", "x:1|1", "x:2|0"] if behind else ["0|1:x", "1|1:x", "2|0:x"]
        cells = [long_col] + short if first else short[:1] + [long_col] + short[1:]
        recs.append(cells)
        fmts.append("XX:GT" if behind else "GT:XX")
        a = 0 if first else len(short[0]) + 1
        claims += [("cols", r, 4), ("no_tab", r, a, a + len(long_col)), ("tab", r, a + len(long_col))]
        tile = 0 if first else TILE
        assert a <= tile and a + len(long_col) >= tile + TILE            # the tile [tile, tile + 4096) holds no tab
    return _case(name, recs, 4, claims, fmts=fmts)


def _a_edge_tabs(name):
    recs = [["", "0|1", "1|0", "1|1", "2|1"], ["0|1", "1|0", "1|1", "2|1", ""], ["", "1|0", "1|1", "2|1", ""], ["", "", "", "", ""],
            ["", "1", "2", "3", "1"], ["1", "2", "3", "1", ""]]
    claims = []
    for r, cells in enumerate(recs):
        claims += [("cols", r, 5)] + ([("tab", r, 0)] if cells[0] == "" else []) + ([("tab", r, -1)] if cells[-1] == "" else [])
    return _case(name, recs, 5, claims + [("span_len", 3, 4)])


def _a_five_tiles(name):
    rng = _rng(name)
    forms = ["0|0", "0|1", "1|0", "1/1", "2|3", "./.", "0/0", "3|3"]
    cells = list(rng.choice(forms, size=5000, p=[0.6, 0.1, 0.1, 0.05, 0.05, 0.03, 0.04, 0.03]))
    return _case(name, [cells, ["0|1"] * 5000], 5000, [("span_len", 0, 19999), ("cols", 0, 5000), ("cols", 1, 5000)])


# ---- B: widths and keep masks ----------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513)
_MIXED = ["0|0", "0|1", "1|0", "0/0", "0/1", "2|3", "./.", ".|1", "1/.", "0|1|2", "3", "12|0", "", "."]


def _width_records(rng, n):
    return [list(rng.choice(_MIXED, size=n)),                                            # everything at once, mixed ploidy
            list(rng.choice(["0", "1", ".", "2", "3"], size=n)),                         # ploidy 1: the second allele is the next KEPT sample's
            ["0|0"] * n,                                                                 # no entry at all
            list(rng.choice(["0|1", "1|1", "2|0"], size=n)),                             # every kept sample is an entry
            list(rng.choice(["0|0", "0|1"], size=n, p=[0.9, 0.1]))]


def _b_width(name, n):
    recs = _width_records(_rng(name), n)
    return _case(name, recs, n, [("cols", r, n) for r in range(len(recs))] + [("ploidy", 1, 1), ("ploidy", 2, 2), ("odd_kept", 2, [])])


KEEP_MASKS = ("first", "last", "alternate", "middle")


def keep_mask(kind, n):
    k = np.zeros(n, np.uint8)
    if kind == "first":
        k[0] = 1
    elif kind == "last":
        k[n - 1] = 1
    elif kind == "alternate":
        k[0::2] = 1
    else:
        k[n // 2] = 1
    return k


def _b_keep(name, n, kind):
    recs = _width_records(_rng(name), n)
    return _case(name, recs, n, [("cols", r, n) for r in range(len(recs))] + [("ploidy", 1, 1), ("odd_kept", 2, [])], keep=keep_mask(kind, n))


def _b_compact_seam(name, alternate):
    """records whose only entries are kept samples 255, 256 and 257: the last of the compaction's first tile, the first two of the next"""
    n = 1026 if alternate else 513
    keep = keep_mask("alternate", n) if alternate else None
    col_of = (lambda s: 2 * s) if alternate else (lambda s: s)
    recs, claims = [], []
    for r, odd in enumerate(([255], [256], [257], [255, 256, 257], [0, 512], [])):
        cells = ["0|0"] * n
        for s in odd:
            cells[col_of(s)] = "1|0"
        if alternate:
            for c in range(1, n, 2):
                cells[c] = "1|1"                                         # (the columns that are not kept: entries, were they read)
        recs.append(cells)
        claims.append(("odd_kept", r, odd))
    return _case(name, recs, n, claims + [("default", PHASED0)], keep=keep)


# ---- C: record counts (the persistent loops) -----------------------------------------------------------------------------
RECORD_COUNTS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 3100)


def loop_kind(r):
    """0, 2: ploidy 1; 1: all default; 3: no default.  Alternates from record to record, and moves on by one between the records one
    workgroup of the decode kernel takes in turn (r, r + 1024), by two between those of the compaction (r, r + 2048)"""
    return (r + r // DECODE_GRID) % 4


def loop_record(r, n):
    """record r of a family-C batch: consecutive records, and records a grid apart, differ in everything a workgroup carries over"""
    if r % 5 == 4:
        return None                                                      # no sample column at all
    kind = loop_kind(r)
    if kind == 1:
        cells = ["0|0"] * n                                              # all default
    elif kind == 3:
        cells = ["%d|%d" % (1 + (r + c) % 60, 1 + (r // 7 + c) % 100) for c in range(n)]        # no default; maxima and masks move with r
    else:
        cells = ["%d" % (1 + (r // 2 + 3 * c) % 50) for c in range(n)]                          # ploidy 1
    if r % 3 == 2:
        cells = cells[:1 + (r // 3) % (n - 1)] if n > 1 else cells       # shorter than the header: the missing columns read "."
    return cells


def _c_records(name, n_records, n_columns, keep):
    recs = [loop_record(r, n_columns) for r in range(n_records)]
    claims = []
    for r, cells in enumerate(recs):
        if cells is None or len(cells) < n_columns:
            claims.append(("cols", r, 0 if cells is None else len(cells)))
        elif loop_kind(r) in (0, 2):
            claims.append(("ploidy", r, 1))
        elif loop_kind(r) == 1:
            claims.append(("odd_kept", r, []))
        else:
            claims.append(("ploidy", r, 2))
    return _case(name, recs, n_columns, claims, keep=keep)


# ---- D: token forms ---------------------------------------------------------------------------------------------------------
LONG_GT = "|".join("%d" % (i % 4) for i in range(300))                   # 300 values: the count saturates at 255
FORMS = ("0", ".", "", "0|0", "0/0", ".|.", "./1", "1|.", "0|1|2", "0/1|2", "007", "63", "64", "127", "63|64", "127/126", "64/1", LONG_GT)
# (form, largest allele number in it): the forms a panel record with that many ALT alleles may carry
PANEL_FORMS = (("0", 0), (".", 0), ("", 0), ("0|0", 0), ("0/0", 0), (".|.", 0), ("./1", 1), ("1|.", 1), ("0|1|2", 2), ("0/1|2", 2), ("001", 1), ("01|00", 1),
               ("1", 1), ("2/1", 2), ("3|2", 3), ("|".join("%d" % (i % 2) for i in range(300)), 1))


def _d_forms(name, n, keep):
    """every form as the first, the middle and the last kept column, among diploid neighbours and among ploidy-1 ones"""
    kept = list(range(n)) if keep is None else [int(c) for c in np.flatnonzero(keep)]
    recs, claims = [], []
    for f in FORMS:
        for at in (kept[0], kept[len(kept) // 2], kept[-1]):
            for fill in ("1|2", "3"):
                cells = [fill] * n
                cells[at] = f
                claims.append(("odd_kept", len(recs), [] if f == fill else [kept.index(at)]))
                recs.append(cells)
    return _case(name, recs, n, claims, keep=keep)


def _d_gt_index(name, gi):
    fmt = ":".join(["K%d" % i for i in range(gi)] + ["GT", "ZZ"])
    recs = []
    for r in range(4):
        recs.append(["x:" * gi + f + (":y" if (r + c) % 2 else "") for c, f in enumerate(FORMS[3 * r:3 * r + 3] + FORMS[12 - r:13 - r])])
    return _case(name, recs, 4, [("gt_index", r, gi) for r in range(4)] + [("cols", r, 4) for r in range(4)], fmts=fmt)


def _d_short_columns(name):
    """FORMAT AA:BB:GT:CC: columns that stop one sub-field short of GT, exactly at its ':', before that, and whole ones"""
    forms = ["a:b", "a:b:", "a", "a:b:1|0:c", "a:b:2/1", "", "a:", "a:b:3"]
    recs = []
    for r in range(len(forms)):
        recs.append([forms[(r + c) % len(forms)] for c in range(5)])
    recs.append(["a:b", "a:b:", "a", "a:", ""])                           # nothing but columns without a GT
    recs.append(["a:b:1", "a:b", "a:b:2", "a:b:", "a:b:3"])              # ploidy 1 between them
    return _case(name, recs, 5, [("gt_index", r, 2) for r in range(len(recs))], fmts="AA:BB:GT:CC")


# ---- E: largest allele ---------------------------------------------------------------------------------------------------------
BIG_ALLELES = ("128", "32767", "32768", "1000001", "1234567890123456789012345")
BIG_MAX = (128, 32767, 32767, 32767, 32767)


def _e_largest(name):
    recs, beyond = [], []
    for i, a in enumerate(BIG_ALLELES):
        for cells in (["0|1", a + "|1", "2|0", "1|1"], ["0|1", "1|0", "2|0", "3/" + a], ["1", "2", a, "3"]):
            recs.append(["1|2", "0|0", "3|1", "0/1"])                    # its neighbours in the batch: undisturbed
            if int(a) > 32767:
                beyond.append(len(recs))
            recs.append(cells)
    recs.append(["2|2", "0|0", "3|1", "0/1"])
    return _case(name, recs, 4, [("max_only", beyond)])


# ---- F: the default word -------------------------------------------------------------------------------------------------------
def _f_default(name, phased0, unphased0, default):
    cells = ["0|0"] * phased0 + ["0/0"] * unphased0 + ["0|1", "1/0", "1|1"]
    _rng(name).shuffle(cells)
    n = 7
    while len(cells) % n:
        cells.append("1|0")
    recs = [cells[a:a + n] for a in range(0, len(cells), n)]
    return _case(name, recs, n, [("zero_words", phased0, unphased0), ("default", default)])


def _f_only_unphased(name):
    return _case(name, [["0/0"] * 6] * 5, 6, [("zero_words", 0, 30), ("default", 0)] + [("odd_kept", r, []) for r in range(5)])


# ---- G: where the spans lie ----------------------------------------------------------------------------------------------------
def _g_records(name, n=9, width=6):
    rng = _rng(name)
    return [list(rng.choice(_MIXED[:9], size=width)) if r % 4 != 3 else list(rng.choice(["0", "1", "2"], size=width)) for r in range(n)]


def _g_offset(name):
    return _case(name, _g_records(name), 6, [("text_off", 0, 1 << 20)], pad_header=1 << 20)


def _g_descending(name):
    return _case(name, _g_records(name), 6, [("select", list(range(8, -1, -1)))])


def _g_shared(name):
    return _case(name, _g_records(name), 6, [("select", [0, 0, 1, 3, 3, 3, 2, 0])])


def _g_all_empty(name):
    recs = [None, [""], None, None, [""], None]
    return _case(name, recs, 4, [("span_len", r, 0) for r in range(len(recs))])


def _g_zero_records(name):
    return _case(name, _g_records(name), 6, [("select", [])])


# ---- the cases --------------------------------------------------------------------------------------------------------------
CASES = {}
for _behind in (False, True):
    _sfx = "-gt-behind" if _behind else "-gt-in-front"
    CASES["A-span-lengths" + _sfx] = functools.partial(_a_span_lengths, behind=_behind)
    CASES["A-tab-last-of-piece-wave-tile" + _sfx] = functools.partial(_a_seam, where=-1, behind=_behind)
    CASES["A-tab-first-of-piece-wave-tile" + _sfx] = functools.partial(_a_seam, where=0, behind=_behind)
CASES["A-sixteen-tabs"] = _a_sixteen_tabs
CASES["A-tile-without-tab"] = _a_tile_without_tab
CASES["A-edge-tabs"] = _a_edge_tabs
CASES["A-five-tiles"] = _a_five_tiles
for _n in WIDTHS:
    CASES["B-width-%d" % _n] = functools.partial(_b_width, n=_n)
for _n in (300, 513):
    for _kind in KEEP_MASKS:
        CASES["B-keep-%d-%s" % (_n, _kind)] = functools.partial(_b_keep, n=_n, kind=_kind)
CASES["B-compact-seam"] = functools.partial(_b_compact_seam, alternate=False)
CASES["B-compact-seam-alternate-kept"] = functools.partial(_b_compact_seam, alternate=True)
_KEEP3 = [1, 0, 1, 0, 1]
for _n in RECORD_COUNTS:
    CASES["C-records-%d" % _n] = functools.partial(_c_records, n_records=_n, n_columns=5, keep=_KEEP3)
CASES["C-records-1100-wide-300"] = functools.partial(_c_records, n_records=1100, n_columns=300, keep=None)
CASES["D-forms"] = functools.partial(_d_forms, n=5, keep=None)
CASES["D-forms-kept-3-of-7"] = functools.partial(_d_forms, n=7, keep=[0, 1, 0, 1, 0, 1, 0])
for _gi in (0, 1, 5, MAX_GT_INDEX):
    CASES["D-gt-index-%d" % _gi] = functools.partial(_d_gt_index, gi=_gi)
CASES["D-short-columns"] = _d_short_columns
CASES["E-largest-allele"] = _e_largest
CASES["F-phased-one-more"] = functools.partial(_f_default, phased0=12, unphased0=11, default=PHASED0)
CASES["F-tie"] = functools.partial(_f_default, phased0=11, unphased0=11, default=PHASED0)
CASES["F-phased-one-fewer"] = functools.partial(_f_default, phased0=10, unphased0=11, default=0)
CASES["F-only-unphased"] = _f_only_unphased
CASES["G-first-span-1MB-in"] = _g_offset
CASES["G-descending-spans"] = _g_descending
CASES["G-shared-spans"] = _g_shared
CASES["G-all-spans-empty"] = _g_all_empty
CASES["G-zero-records"] = _g_zero_records

LOOP_TWICE = ("C-records-3100", "C-records-1025")     # on one context, in this order: the larger batch's scratch must not leak


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name](name)


def runs():
    """(case name, haploid) for every mode of every case"""
    return [(name, h) for name in CASES for h in get(name).modes]


# ---- H: what mg_decode_gt_text refuses -----------------------------------------------------------------------------------------
def _h_span_past_end(a):
    a["ln"] = a["ln"].copy()
    a["ln"][-1] = len(a["raw"]) - int(a["off"][-1]) + 1


def _h_index(a, value):
    a["gi"] = a["gi"].copy()
    a["gi"][len(a["gi"]) // 2] = value


def _h_no_columns(a):
    a["n_columns"], a["keep"] = 0, None


def _h_keep_nothing(a):
    a["keep"] = np.zeros(a["n_columns"], np.uint8)


REFUSALS = {"H-span-past-the-text": _h_span_past_end, "H-gt-index-minus-1": functools.partial(_h_index, value=-1),
            "H-gt-index-1001": functools.partial(_h_index, value=MAX_GT_INDEX + 1), "H-no-columns": _h_no_columns, "H-keep-mask-of-zeros": _h_keep_nothing}
REFUSALS_OVER = "G-descending-spans"      # the valid batch each refusal spoils, and which is decoded again afterwards


# ---- the claims, read back from the bytes ---------------------------------------------------------------------------------------
def check_claims(case, directory):
    """every claim of the case against the bytes `_spans` returns -> the kinds of claim that were checked"""
    path = os.path.join(directory, "claims.vcf")
    _write(path, case.records, case.n_columns, lambda i: case.fmts[i], pad_header=case.pad_header)
    raw, off, ln, gi = _spans(path)
    span = lambda r: raw[int(off[r]):int(off[r]) + int(ln[r])]
    kept = list(range(case.n_columns)) if case.keep is None else [int(c) for c in np.flatnonzero(case.keep)]

    def gts(r):          # the GT strings of record r's kept columns (absent columns and sub-fields: ".")
        cols = span(r).split(b"\t") if ln[r] else []
        out = []
        for c in kept:
            fields = cols[c].split(b":") if c < len(cols) else [b"."]
            out.append(fields[gi[r]] if gi[r] < len(fields) else b".")
        return out

    seen = set()
    for c in case.claims:
        kind, a = c[0], c[1:]
        seen.add(kind)
        if kind == "records":
            assert len(off) == a[0] == len(case.records)
        elif kind == "span_len":
            assert ln[a[0]] == a[1], c
        elif kind == "tab":
            assert span(a[0])[a[1]:][:1] == b"\t", c
        elif kind == "no_tab":
            assert a[1] < a[2] <= ln[a[0]] and b"\t" not in span(a[0])[a[1]:a[2]], c
        elif kind == "cols":
            n = span(a[0]).count(b"\t") + 1 if ln[a[0]] else (1 if case.records[a[0]] is not None else 0)
            assert n == a[1] <= case.n_columns, c
        elif kind == "gt_index":
            assert gi[a[0]] == a[1], c
        elif kind == "ploidy":
            assert max(len(g.replace(b"/", b"|").split(b"|")) for g in gts(a[0])) == a[1], c
        elif kind == "zero_words":
            every = [g for r in range(len(off)) for g in gts(r)]
            assert (every.count(b"0|0"), every.count(b"0/0")) == tuple(a), c
            assert all(g in (b"0|0", b"0/0") or set(g.replace(b"/", b"|").split(b"|")) - {b"0", b".", b""} for g in every), c
            assert all(len(g.replace(b"/", b"|").split(b"|")) == 2 for g in every), c     # (a lone "0" in a diploid record is 0|0 too)
        elif kind == "odd_kept":
            g = gts(a[0])
            common = Counter(g).most_common(1)[0][0]
            assert [s for s, x in enumerate(g) if x != common] == list(a[1]), c
        elif kind == "text_off":
            assert off[a[0]] >= a[1], c
        elif kind == "select":
            assert all(0 <= r < len(off) for r in a[0]), c
        elif kind == "max_only":
            for r in range(len(off)):
                big = max([int(t) for g in gts(r) for t in g.replace(b"/", b"|").split(b"|") if t not in (b"", b".")] + [0])
                assert (big > 32767) == (r in a[0]), c
        elif kind == "default":
            assert a[0] in (0, PHASED0), c
        else:
            raise AssertionError("unknown claim %r" % (c,))
    return seen

