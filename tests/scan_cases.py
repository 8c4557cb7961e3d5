"""Directed cases for the call-time k-mer scan (csrc/scan_kernels.h; scan_plan / launch_scan_chunk in csrc/malva_hip.hip): the
direct, ticket, sub-slice and partition forms at their seams.  No GPU and no product import here: tests/test_scan_cases_cpu.py
checks on any machine that every case holds what its name says and that the plain-Python restatement of the plan arithmetic below
gives the form, layout and spill count the case claims; tests/test_gpu_scan_edges.py hands the same cases to the device.

A case is a name, the seam it aims at, a Setup (k, ref_k, filter bits, gate), the options to set, which pool rows are indexed
and where, the table as an ORDER over a pool of at most a few thousand distinct rows, the entry it goes through, and its claims.

The multiplicity identity.  The scan adds, for every table row, the row's count to at most one exact-map value (wrapping at
2^32, kmap.hpp:114-122) and at most one filter counter (a u16 cell keeping the low 16 bits, bloom_filter.hpp:100-113); whether it
does depends on the row's k-mers and on the index alone, never on the counters.  Wrapping adds commute and 2^16 divides 2^32, so a
table holding pool row i m_i times leaves what ONE scan of the pool with the counts (c_i * m_i) mod 2^32 leaves: a table of
millions of rows costs the oracle the pool.  expected() does that; the CPU file proves it against a row-by-row oracle scan.

Pool rows are random ref_k-mers of a seeded generator; where a row must sit in a chosen slot, gate word, slice, sub-slice or bin
it is FOUND with the oracle's hash (mo_bf_hash of the centre k-mer, canonicalised by the oracle) and the arithmetic below -- by
selecting on the seeded pool's slots, or for single slots by a larger seeded search whose finds are recorded as literals
(SLOT_ROWS, H_PAIR).  The CPU file computes the slot of EVERY pool row of every setup again, one k-mer at a time and by another
route (mo_canonical, then mo_xxh3_64), so every selection by word, slice, sub-slice or bin rests on verified slots; a sample of
each pool and every literal goes through a third route as well (a fresh oracle filter's add_key).

Of a seeded pool only the rows whose fine-gate word is EVEN are indexed; the rows of odd words find their gate word empty, so
they are closed whatever the gate's false-positive rate.  model() bounds the open rows of the last launch group from that: a
row that shares its slot with an indexed row is open, a row whose gate word holds no indexed row is closed, any other row may be
either -- in nearly every case there is none of those and the bound is an equality.  The rows whose slot is a set bit of `bf`
(n_hits, whole call) are counted from the oracle's words, and the tickets that spill are exact (every row is filed).

The restated arithmetic (line numbers: csrc/malva_hip.hip unless a file is named):
    gate            alloc_gate 400-425     shift S >= 6 smallest with ceil(size / 2^S) <= 2^gate_log2; word = slot >> (S + 6)
    slices          ticket_slices 1379     word_shift = pregate_log2 - 7; slice = word >> word_shift
    sub-slices      sub_bins 1442          bin = slot >> (S + 6 + sub_words_log2)
    form, chunk     scan_plan 1506-1541
    ticket layout   ticket_layout 1385     nseg = min(ceil(cap / 1024), 2048); segcap; launch: workgroup w takes the 2,048-row tiles
                                           w, w + nseg, ... (scan_kernels.h:753)
    sub layout      sub_layout 1448        nseg = min(tiles, sub_grid or CUs); parts; ucap; 16,384-row tiles dealt the same way
                                           (scan_kernels.h:1059); a tile is "slow" when a segment would overflow (1133)
    spilled         what a segment cannot take: sum over (bin, workgroup) of max(0, fill - segcap) (scan_kernels.h:836-837, 1147-1148)
    direct          launch_filter_var 1570 tile T = 256 * scan_rows, grid = min(ceil(n / T), scan_grid); stage CAP = T + 256,
                                           flushed when more than 256 are staged (scan_kernels.h:301, 376)
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import capi as ocapi

U = np.uint64
TPB = 256
TK_TILE, TK_MAXP, BIN_SEGS, BIN_MAXP = 2048, 256, 2048, 32
TKG_SPW, TKG_WSTAGE, TKG_STEP = 64, 2048, 8 * 512
SB_TILE, SB_MAXB, SB_WORDS_LOG2, SBG_STEP = 16384, 1024, 14, 640
CUS = 256                                     # an MI355X; the GPU file passes the device's own count to the model

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_CODE = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def revcomp(s):
    return s[::-1].translate(_COMP)


def hashes(kmers):
    """BF::_get_hash of each k-mer, from the oracle (never from the device)"""
    f = ocapi.lib().mo_bf_hash
    return np.array([f(km) for km in kmers], dtype=U)


def pack(rk):
    """uint8 [n, L] ASCII -> (hi, lo): base i at bits 2 (L - 1 - i) of the 128-bit value (the table's M-form)"""
    codes = _CODE[rk].astype(U)
    n, L = rk.shape
    hi, lo = np.zeros(n, dtype=U), np.zeros(n, dtype=U)
    for i in range(L):
        sh = 2 * (L - 1 - i)
        if sh >= 64:
            hi |= codes[:, i] << U(sh - 64)
        else:
            lo |= codes[:, i] << U(sh)
    return hi, lo


# ---- the restated arithmetic ------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return (a + b - 1) // b


def gate_geometry(bits, gate_log2):
    """(shift, gate bits, gate words)"""
    s = 6
    while ceil_div(bits, 1 << s) > (1 << gate_log2):
        s += 1
    ngb = ceil_div(bits, 1 << s)
    return s, ngb, ceil_div(ngb, 64)


DEFAULTS = dict(use_summary=1, use_sub=1, sub_min_log2=28, sub_words_log2=SB_WORDS_LOG2, use_tickets=1, ticket_min_log2=28, use_pregate=1,
                use_partition=0, scan_chunk_log2=27, scan_bin_cap=0, sub_grid=0, scan_rows=2, scan_variant=2, scan_grid=8192,
                pregate_log2=25, gate_log2=25)


def plan(bits, opts, n, rows12, cus=CUS):
    """scan_plan + the form's layout for a table of n rows: a dict with form, chunk, nbins and the layout's numbers"""
    o = dict(DEFAULTS)
    o.update(opts)
    shift, ngb, nwords = gate_geometry(bits, o["gate_log2"])
    idx_bits = 1
    while idx_bits < 64 and (bits - 1) >> idx_bits:
        idx_bits += 1
    row_bits = min(27, 64 - idx_bits)
    two_pass = bool(o["use_summary"]) and idx_bits <= 44
    word_shift = o["pregate_log2"] - 7
    TP = ceil_div(nwords, 1 << word_shift)
    NB = ceil_div(nwords, 1 << o["sub_words_log2"])
    has_pregate = o["gate_log2"] > o["pregate_log2"]
    if two_pass and o["use_sub"] and o["gate_log2"] >= o["sub_min_log2"] and 2 <= NB <= SB_MAXB:
        form = "subs"
    elif two_pass and o["use_tickets"] and o["gate_log2"] >= o["ticket_min_log2"] and 2 <= TP <= TK_MAXP:
        form = "tickets"
    elif not rows12 and has_pregate and o["use_summary"] and o["use_pregate"] and o["use_partition"] and 2 <= TP <= BIN_MAXP:
        form = "bins"
    else:
        form = "direct"
    chunk = 1 << min(row_bits if form in ("tickets", "subs") else 27, o["scan_chunk_log2"])
    if rows12:
        chunk = max(4, chunk)
    cap = min(n, chunk)
    p = dict(form=form, chunk=chunk, cap=cap, shift=shift, nwords=nwords, row_bits=row_bits, nbins=0)
    if form == "tickets":
        nseg = min(ceil_div(cap, 4 * TPB), BIN_SEGS)
        wg_rows = ceil_div(ceil_div(cap, TK_TILE), nseg) * TK_TILE
        p.update(nbins=TP, bin_shift=shift + 6 + word_shift, tile=TK_TILE, nseg=nseg, seg_rows=4 * TPB,
                 segcap=o["scan_bin_cap"] or ((wg_rows // TP) * 3 // 2 + 64 + 15) // 16 * 16)
    elif form == "subs":
        tiles = ceil_div(cap, SB_TILE)
        nseg = min(tiles, min(o["sub_grid"], SB_MAXB) if o["sub_grid"] > 0 else cus)   # (mg_set_option clamps sub_grid to SB_MAXB)
        wg_rows = ceil_div(tiles, nseg) * SB_TILE
        segcap = o["scan_bin_cap"] or ((wg_rows // NB) * 3 // 2 + 64 + 15) // 16 * 16
        parts = max(1, min(8, nseg, cus // NB))
        p.update(nbins=NB, bin_shift=shift + 6 + o["sub_words_log2"], tile=SB_TILE, nseg=nseg, seg_rows=SB_TILE, segcap=segcap,
                 parts=parts, ucap=ceil_div(nseg, parts) * segcap)
    elif form == "bins":
        p.update(nbins=TP, bin_shift=shift + 6 + word_shift, nseg=min(ceil_div(cap, 2 * TPB), BIN_SEGS))
    return p


def last_chunk(p, n):
    """(first row, rows) of the last launch group"""
    r0 = (n - 1) // p["chunk"] * p["chunk"]
    return r0, n - r0


def fills(p, slots_of_chunk):
    """[nbins, launched workgroups] tickets pass one files per segment before the capacity is applied: workgroup w of the
    launch takes the tiles w, w + nseg, ... of the launch group"""
    nr = len(slots_of_chunk)
    nseg = min(ceil_div(nr, p["seg_rows"]), p["nseg"])
    wg = (np.arange(nr) // p["tile"]) % nseg
    b = (slots_of_chunk >> U(p["bin_shift"])).astype(np.int64)
    return np.bincount(b * nseg + wg, minlength=p["nbins"] * nseg).reshape(p["nbins"], nseg)


def spilled(p, slots_of_chunk):
    return int(np.maximum(fills(p, slots_of_chunk) - p["segcap"], 0).sum())


def sub_tile_modes(p, slots_of_chunk):
    """per launched workgroup of scan_sub_sort_kernel, a string with one letter per tile it takes: F = left waiting and stored
    during the next tile's hashing (or after the loop), S = a segment would overflow: stored at once, through the spill list"""
    nr = len(slots_of_chunk)
    nseg = min(ceil_div(nr, SB_TILE), p["nseg"])
    out = []
    for w in range(nseg):
        pos = np.zeros(p["nbins"], dtype=np.int64)
        modes = ""
        for base in range(w * SB_TILE, nr, nseg * SB_TILE):
            mine = np.bincount((slots_of_chunk[base:base + SB_TILE] >> U(p["bin_shift"])).astype(np.int64), minlength=p["nbins"])
            modes += "S" if (pos + mine > p["segcap"]).any() else "F"
            pos = np.minimum(pos + mine, p["segcap"])
        out.append(modes)
    return out


def direct_stage_trace(n, rows, grid, opened):
    """scan_filter_kernel's stage, per workgroup: the staged count after every iteration, before flush_if_above(256) looks at it"""
    T = TPB * rows
    g = min(ceil_div(n, T), grid)
    out = []
    for w in range(g):
        staged, seen = 0, []
        for base in range(w * T, n, g * T):
            staged += int(opened[base:base + T].sum())
            seen.append(staged)
            if staged > 256:
                staged = 0
        out.append(seen)
    return out


def ticket_walks(p, fill, grid):
    """scan_ticket_gate_kernel 955-964: (workgroup, slice, first segment, segments, tickets) of every walk"""
    P, nseg, out = p["nbins"], fill.shape[1], []
    for b in range(grid):
        xcd, local, nlocal = b & 7, b >> 3, grid >> 3
        nshare = 1 if P >= 8 else (8 - xcd % P + P - 1) // P
        me = local if P >= 8 else local * nshare + xcd // P
        spw = ceil_div(nseg, nlocal * nshare)
        s0 = me * spw
        s1 = min(s0 + spw, nseg) if s0 < nseg else s0
        for sl in range(xcd if P >= 8 else xcd % P, P, 8):
            for s in range(s0, s1, TKG_SPW):
                k = min(TKG_SPW, s1 - s)
                out.append((b, sl, s, k, int(np.minimum(fill[sl, s:s + k], p["segcap"]).sum())))
    return out


def map_records(bits, n_keys, n_set, slots):
    """home record of filter slots in an ORDERED map (option map_ordered): map_reserve 474-478 sizes the table, map_home
    (kmer_dev.h:411) scales the slot onto it"""
    want = 10
    while (1 << want) < n_keys * 4 or (1 << want) < n_set * 2:
        want += 1
    mul = ((1 << 64) - 1) // bits
    return [((int(s) * mul) & ((1 << 64) - 1)) >> (64 - want) for s in slots]


# ---- setups: a filter, its gate, a seeded pool -------------------------------------------------------------------------------
class Setup:
    """kinds of the indexed (even-word) pool rows, by their place among them: 0 -> bf, 1 -> exact map, 2 -> both, 3 -> bf and the
    row's ref_k-mer in context_bf (the row is blocked, main.cpp:496).  Rows of odd gate words are not indexed: closed."""

    def __init__(self, k, ref_k, bits, gate_log2, pregate_log2=25, n_pool=4096, seed=1, ctx="insert"):
        self.k, self.ref_k, self.bits, self.gate_log2, self.pregate_log2, self.ctx = k, ref_k, bits, gate_log2, pregate_log2, ctx
        self.off = (ref_k - k) // 2
        self.shift, self.ngb, self.nwords = gate_geometry(bits, gate_log2)
        rng = np.random.default_rng([seed, k, ref_k, bits % 1000003])
        self.rk = np.zeros((0, ref_k), dtype=np.uint8)
        self.rkmers, self.centres = [], []
        self.slot, self.hi, self.lo = np.zeros(0, dtype=U), np.zeros(0, dtype=U), np.zeros(0, dtype=U)
        self.cnt, self.kind = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64)
        self.extend([bytes(r) for r in _ACGT[rng.integers(0, 4, size=(n_pool, ref_k))]])
        self.open = np.flatnonzero(self.word % 2 == 0)         # (of the seeded rows: extend() leaves these two alone)
        self.closed = np.flatnonzero(self.word % 2 == 1)
        self.kind[self.open] = np.arange(len(self.open)) % 4

    @property
    def word(self):
        return (self.slot >> U(self.shift + 6)).astype(np.int64)

    def extend(self, rkmers, counts=None):
        """more pool rows (the seeded ones, then found or constructed ones) behind those there are; returns their pool indices.
        New rows are not indexed (kind -1) until the caller gives them a kind."""
        first = len(self.rkmers)
        add = np.array([np.frombuffer(r, dtype=np.uint8) for r in rkmers], dtype=np.uint8).reshape(len(rkmers), self.ref_k)
        centres = [r[self.off:self.off + self.k] for r in rkmers]
        hi, lo = pack(add)
        self.rk = np.concatenate([self.rk, add])
        self.rkmers += list(rkmers)
        self.centres += centres
        self.slot = np.concatenate([self.slot, hashes(centres) % U(self.bits)])
        self.hi, self.lo = np.concatenate([self.hi, hi]), np.concatenate([self.lo, lo])
        new = np.arange(first, len(self.rkmers))
        self.cnt = np.concatenate([self.cnt, (1 + (new * 37) % 255).astype(np.uint32) if counts is None else np.asarray(counts, dtype=np.uint32)])
        self.kind = np.concatenate([self.kind, np.full(len(new), -1, dtype=np.int64)])
        return new

    def index_lists(self, rows=None):
        """(bf k-mers, map k-mers, ref_k-mers for context_bf) of the indexed rows among `rows` (default: the whole pool)"""
        rows = np.arange(len(self.rkmers)) if rows is None else np.asarray(rows)
        kd = self.kind[rows]
        pick = lambda ks: [int(i) for i in rows[np.isin(kd, ks)]]
        return pick([0, 2, 3]), pick([1, 2]), pick([3])

    def options(self):
        return [("gate_log2", self.gate_log2)] + ([("pregate_log2", self.pregate_log2)] if self.pregate_log2 != 25 else [])


def _with_slot_rows(G):
    """the recorded rows of SLOT_ROWS behind the seeded ones: per slot a bf row, one that is a map key too and a blocked one, then the
    blocked rows' twins -- the same centre k-mer under another context (they differ in the first base only)"""
    G.slot_rows = {}
    for s in SLOT_TARGETS:
        G.slot_rows[s] = G.extend(SLOT_ROWS[s])
        G.kind[G.slot_rows[s]] = [0, 2, 3]
    twins = [(b"A" if r[:1] != b"A" else b"C") + r[1:] for r in (G.rkmers[G.slot_rows[s][2]] for s in SLOT_TARGETS)]
    G.twins = G.extend(twins)
    G.kind[G.twins] = -2                                        # not indexed themselves: they hit through their twin's bit
    return G


def _with_palindromes(E):
    """40 rows whose centre k-mer (k even) is its own reverse complement; those of even gate words are indexed like the seeded rows"""
    rng = np.random.default_rng(34)
    half_n, flank_n = E.k // 2, E.ref_k - E.k
    pal = []
    for _ in range(40):
        half = bytes(_ACGT[rng.integers(0, 4, size=half_n)])
        flank = bytes(_ACGT[rng.integers(0, 4, size=flank_n)])
        pal.append(flank[:E.off] + half + revcomp(half) + flank[E.off:])
    E.pal = E.extend(pal)
    even = E.pal[E.word[E.pal] % 2 == 0]
    E.kind[even] = np.arange(len(even)) % 4
    return E


H_PAIR = (3070, 3395, 4)                       # what find_h_pair() finds in the "std" pool: two bf rows and a map row
H_BF_COUNTS = [65535, 65536, 65537, 1, 0, 0xFFFFFFFF, 31071, 31072, 31073, 7]
H_MAP_COUNTS = [(1 << 31) - 1, 1, 1 << 31, 0xFFFFFFFF, 0]


def hit_rows_of(S):
    """the seeded rows whose slot is a set bit of bf and which context_bf does not block"""
    return unblocked(S, S.open[np.isin(S.kind[S.open], [0, 2])])


def find_h_pair(S):
    """how H_PAIR was made: two bf rows whose slots are the only two set bits of ONE record of an ordered map (map_ordered 1; the
    record before it holds at most two, so nothing walks in) -- entries 0 and 1 of the record, the two 16-bit halves of one word --
    and the first row that is an exact-map key only.  The CPU file holds H_PAIR to this search and to the record arithmetic."""
    hit_rows = hit_rows_of(S)
    bf_i, mp_i, _ = S.index_lists()
    pos = np.unique(S.slot[bf_i])
    rec = np.array(map_records(S.bits, len(mp_i), len(pos), pos))
    per = dict(zip(*(x.tolist() for x in np.unique(rec, return_counts=True))))
    for r in sorted(per):
        rows2 = [int(hit_rows[np.flatnonzero(S.slot[hit_rows] == q)[0]]) for q in pos[rec == r] if (S.slot[hit_rows] == q).any()]
        if per[r] == 2 and per.get(r - 1, 0) <= 2 and len(rows2) == 2:
            return rows2[0], rows2[1], int(S.open[S.kind[S.open] == 1][0])
    raise LookupError("no record with exactly two entries")


def _with_counter_rows(S):
    """copies of the H_PAIR rows with chosen counts (the pool's own keep theirs): S.h[("bf", count)] = [copy of the first bf row, of
    the second], S.h[("map", count)] = [copy of the map row]"""
    hrow, hrow2, hmap = S.h_pair = H_PAIR
    nb, nm = len(H_BF_COUNTS), len(H_MAP_COUNTS)
    new = S.extend([S.rkmers[hrow]] * nb + [S.rkmers[hrow2]] * nb + [S.rkmers[hmap]] * nm, H_BF_COUNTS + H_BF_COUNTS + H_MAP_COUNTS)
    S.kind[new] = -2                                            # not indexed themselves: they meet the indexed row's bit or key
    S.h = {("bf", c): [int(new[i]), int(new[nb + i])] for i, c in enumerate(H_BF_COUNTS)}
    S.h.update({("map", c): [int(new[2 * nb + i])] for i, c in enumerate(H_MAP_COUNTS)})
    return S


@functools.lru_cache(maxsize=None)
def setup(name):
    """every pool is complete when this returns: nothing extends it afterwards"""
    if name == "std":                          # 2^20 filter bits, 256 gate words of 4,096 slots: direct form, sub-slices of 2^w words
        return _with_counter_rows(Setup(35, 43, 1 << 20, 20))
    if name == "std-refscan":                  # the same, context_bf filled by the reference scan over the blocked rows' ref_k-mers
        return Setup(35, 43, 1 << 20, 20, ctx="refscan")
    if name == "sub-partial":                  # 255 gate words: with 8-word sub-slices the last of 32 bins holds 7
        return Setup(35, 43, (1 << 20) - 5000, 20)
    if name == "sub-1024":                     # 1,024 gate words, one per sub-slice: the most bins the form takes
        return Setup(35, 43, 1 << 22, 20, n_pool=8192)
    if name.startswith("tk-"):                 # P slices of two gate words (pregate_log2 8), the last one partial where P is odd
        P = int(name[3:])
        words = {2: 4, 3: 5, 5: 10, 7: 13, 9: 18, 256: 512}[P]
        return Setup(35, 43, words * 4096 - (100 if words % 2 else 0), 30, pregate_log2=8, n_pool=8192 if P == 256 else 4096)
    if name == "part-32":                      # partition form: 32 slices of 8 words behind a 2^10-bit coarse gate
        return Setup(35, 43, 1 << 20, 14, pregate_log2=10)
    if name == "part-2":
        return Setup(35, 43, 1 << 16, 11, pregate_log2=10)
    if name == "k34-44":                       # an even k: palindromic centre k-mers
        return _with_palindromes(Setup(34, 44, 1 << 20, 20))
    if name == "k34-44-tk":                    # the same through 5 ticket slices (as tk-5)
        return _with_palindromes(Setup(34, 44, 10 * 4096, 30, pregate_log2=8))
    if name.startswith("k"):                   # other (k, ref_k): compact rows of ref_k 33 and 44
        k, r = (int(x) for x in name[1:].split("-"))
        return Setup(k, r, 1 << 20, 20)
    if name == "slots":                        # 2^14 filter bits, 4 gate words; the recorded rows of single slots (SLOT_ROWS)
        return _with_slot_rows(Setup(35, 43, 1 << 14, 20, n_pool=64))
    raise KeyError(name)


SLOT_TARGETS = [0, 4095, 4096, 8191, 8192, 8193, 8194, 8195, 12287, 12288, 16383]


# {slot: [ref_k-mers]} at 2^14 filter bits: slot 0 and size - 1; the last slot of a gate word, slice and sub-slice and the first of
# the next; three adjacent slots of one record.  Found once by find_slot_rows() (1.2e5 hashes) and recorded here; the CPU file
# rehashes every one of them and holds the table to the search.
SLOT_ROWS = {
    0: [b'GCGACGGCACACCGCGAGAGAGTATACCCGAGGTAAGGGACAT', b'CCTTTGTCAAGCCCACGCTGTGCTAGGACGCCCACTATCAACC', b'AGGCCTGCGCCAGAGAGTTGGCATTAGCATCATGAGAACTGAG'],
    4095: [b'GCCCACATCCCTGCGGGAGGATAAAACCGGACTCCGCCGTGCA', b'CAGGCCCCGAAGCCCGGTTTTCTGTCAACGTTCATTACTTTGT', b'ACTTCATCGTATCTAGGTTATCACAATTGTACCTCAAGTCTAA'],
    4096: [b'AATACCAGGCACGCCAATATCCAAATGTGAATTCACGTCGCTC', b'GATCTTGAGTTCCTCCTCGTTGATTATGCTTTCGCATCGCTAC', b'CCTCGGAAGCTTCGTATCGCGAGCCGGAGCTGACGCAGTTAGT'],
    8191: [b'ACGGCCTTCCTATGTATATGCCTAATTTTCCTATGGAGGACCC', b'AATGTCGGATCTCTGGATTCCGACTTGCCCCCCGTGTCTGTTA', b'GTTGTCACATTTCTAACTGGCACTGAAAAGATCGTCATCCAAG'],
    8192: [b'TGCCTACAAAGTTATTCTCGCAGCCCGCGCGCCGAAGCTATGT', b'TTTTTGCCTTTTCGGATGGCGGCCTTAACGGGAGTAGCGGTTA', b'CACTTGAGAATGCTCCTACACCGGCTTCTTCGCACTCTCGGTG'],
    8193: [b'GCATGGCTTGCCTCCTTGTCTAGGAATCAGCGGCTACGAACGG', b'ACCTGGTAGCACGGAGATTTGTAACTTTCTCTTTGCCCGCGAA', b'GGATTCAATATGGTCCTATAGTTGGCATATCGTCGATATGGCA'],
    8194: [b'ATGAAGGAATTGACCAACTTAGTAGACTGGGCAGGTTAAACAA', b'GCGGAGGTCGGGTGATTAGCGAGAATAGTAAACAGACCGCCAT', b'GAGTCAGACCGCACTTCAAAAGCGTCCACACGCCCTAAGATCT'],
    8195: [b'ATTCGAGATACTAGACTTAATATAGGGACAAATGCGAGCTCAG', b'TTGCTGCCGTCCATGATAAGCACCACCCAGGTCTCTACGGTTC', b'TACTCGGCGACTTTGTCTATGTTCGTTCCCTAATCAGACTTCG'],
    12287: [b'TCCGTGAGGTCATAACGATGACCCTCCCTGTGCTCGGTGGCAA', b'CAGACTGACGCTGCCCCTTTTATTATAGTTGTAAAAGTAGGCC', b'GGGAGCGTTTCTTCTGTGCCAAGATTACCGCTGTTTCAGGGAA'],
    12288: [b'CGCAGCGGAACGACCAGAGTTTTATATCGTGAAATAAGGAAAA', b'GAGAGACTATTACTCTGAATATCAGTTCCCCACTTCTTCAGAG', b'GCCGTATCCAGGCCGCTGCACCTATTATTTACCTCATCCCAGA'],
    16383: [b'ATCTCACTCACCCGTTCCTTCTACTTAGCTCTCGGCGTATGGA', b'TTCCCAAGAACTTTGAGCCTCCTACAAATGTATTTAAATTATG', b'GGAAATCTGTGAGGCACGTATTTTAACCGGGATGCGCGTGCCG'],
}


def find_slot_rows():
    """how SLOT_ROWS was made: the first three seeded 43-mers whose centre 35-mer hashes to each target slot"""
    found = {s: [] for s in SLOT_TARGETS}
    seed = 770
    while any(len(v) < 3 for v in found.values()):
        rk = _ACGT[np.random.default_rng(seed).integers(0, 4, size=(60000, 43))]
        rows = [bytes(r) for r in rk]
        sl = hashes([r[4:39] for r in rows]) % U(1 << 14)
        for s in SLOT_TARGETS:
            found[s] += [rows[i] for i in np.flatnonzero(sl == s)][:3 - len(found[s])]
        seed += 1
    return found


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case(namedtuple("Case", "name family seam setup opts indexed order_spec entry offset claims seams")):
    """order_spec: the pool index of every table row, or (the tables of millions of rows) a function that makes it: nothing of that
    size is held between uses"""
    __slots__ = ()

    @property
    def order(self):
        o = self.order_spec
        return np.asarray(o() if callable(o) else o, dtype=np.int64)


# indexed: pool rows the index is made of (their kinds decide where they go); order: pool index of every table row
# entry: host (mg_kmc_scan), device (mg_kmc_scan_device), rows12 (mg_kmc_pack_rows_device + mg_kmc_scan_rows_device),
#        rows12-raw (a caller-made buffer whose padding rows hold an indexed k-mer with a count)
# offset: 1 = the device arrays start one row into their allocations (8 bytes for hi / lo, an odd index for cnt): vec_ok false
# claims: form, nbins and whatever else the CPU file proves from the model; seams: the names of SEAMS the case hits
_CASES = {}


def _add(name, family, seam, setup_name, opts, order, entry="device", offset=0, indexed=None, seams=(), **claims):
    assert name not in _CASES, name
    _CASES[name] = Case(name, family, seam, setup_name, tuple(opts), indexed, order if callable(order) else np.asarray(order, dtype=np.int64), entry, offset, claims, tuple(seams))


def unblocked(s, rows):
    """those of `rows` whose ref_k-mer context_bf does not hold, not by a collision either (the slots of the blocked rows' ref_k-mers)"""
    held = hashes([s.rkmers[i] for i in np.flatnonzero(s.kind == 3)]) % U(s.bits)
    return rows[~np.isin(hashes([s.rkmers[i] for i in rows]) % U(s.bits), held)]


def tiled(rows, n):
    return np.resize(np.asarray(rows), n)


def _build():
    S = setup("std")
    every = np.arange(4096)
    hit_rows = hit_rows_of(S)                                   # slot is a set bit of bf, not blocked
    # A: row counts and tiles of the direct form
    for rows in (1, 2, 4):
        T = TPB * rows
        for var in (0, 2):
            for off in (0, 1):
                for n in (1, 2, 3, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1):
                    _add("A-soa-r%d-v%d-o%d-n%d" % (rows, var, off, n), "A", "tile edge of scan_filter_kernel<%d, VAR %d>, bases %s" % (rows, var, "offset by one row" if off else "aligned"),
                         "std", [("scan_rows", rows), ("scan_variant", var)], tiled(every, n), offset=off, form="direct", entry="host" if (rows, var, off) == (2, 2, 0) else "device",
                         seams=["rows-%d" % rows, "variant-%d" % var] + (["unaligned-direct"] if off else []) + (["partial-tile"] if n % T else []))
    for rows in (1, 2, 4):
        T = TPB * rows
        for grid in (1, 2):
            for left in (256, 257)[:1 if rows == 1 else 2]:
                # gate off: every row is staged.  A full tile (flushed where T > 256; at scan_rows 1 it is 256 rows, which stay, and the
                # second tile fills the stage to its capacity of 512), then `left` rows
                n = grid * T + (grid - 1) * T + left if grid == 2 else T + left
                _add("A-carry-r%d-g%d-left%d" % (rows, grid, left), "A", "staged rows left at %d after a flush, gate off" % left, "std",
                     [("scan_rows", rows), ("scan_grid", grid), ("use_summary", 0)], tiled(every, n), form="direct", left=left, seams=["carry-over", "multi-iteration-direct"])
    for left in (256, 257):
        # gate on, every second row open: a tile of 512 rows stages 256 (kept) or 257 (flushed), and the next tile adds to what was kept
        a = np.empty(512, dtype=np.int64)
        a[0::2], a[1::2] = tiled(S.open, 256), tiled(S.closed, 256)
        if left == 257:
            a[1] = S.open[300]
        _add("A-carry-gated-left%d" % left, "A", "a gate that opens every second row: %d staged rows carried into the next iteration" % left, "std",
             [("scan_grid", 1)], np.concatenate([a, a, a[:77]]), form="direct", left=left, seams=["carry-over", "multi-iteration-direct", "gated-carry"])
    for n in (1, 2, 3, 4, 5, 511, 512, 513, 1025):
        _add("A-rows12-n%d" % n, "A", "compact rows, n mod 4 = %d, one workgroup" % (n % 4), "std", [("scan_grid", 1)], tiled(every, n), entry="rows12",
             form="direct", seams=["rows12-nmod4-%d" % (n % 4), "multi-iteration-direct"] if n > 512 else ["rows12-nmod4-%d" % (n % 4)])
    for r in (33, 43, 44):
        _add("A-rows12-maxcount-r%d" % r, "A", "compact rows whose counts are 2^(96 - 2 ref_k) - 1", "k%d-%d" % (33 if r == 33 else 35, r) if r != 43 else "std", [],
             tiled(every, 1027), entry="rows12", form="direct", maxcount=(1 << (96 - 2 * r)) - 1, seams=["rows12-maxcount"])
    for n in (1, 2, 3, 5):
        _add("A-rows12-raw-pad-n%d" % n, "A", "a caller-made compact buffer whose padding rows hold an indexed k-mer with a count: not counted", "std", [],
             tiled(hit_rows, n), entry="rows12-raw", form="direct", seams=["rows12-padding"])
    # B: probe and hit lists
    for he in (0, 1):
        for m in (255, 256, 257, 1023):
            _add("B-allhit-e%d-n%d" % (he, m), "B", "probe_grid 1, hits_grid 1: %d open rows that all hit (staging carry-over of scan_probe_kernel)" % m, "std",
                 [("probe_grid", 1), ("hits_grid", 1), ("use_hit_entries", he), ("use_record_counters", 2)], tiled(hit_rows, m), all_hit=True, form="direct",
                 seams=["probe-carry", "hit-entries-%d" % he])
    _add("B-open0", "B", "no row passes the gate: open list and hit list of length 0", "std", [("probe_grid", 1)], tiled(S.closed, 700), form="direct", seams=["open-0"])
    _add("B-hit0", "B", "open rows that are exact-map keys only: hit list of length 0", "std", [("probe_grid", 1)],
         tiled(S.open[S.kind[S.open] == 1], 700), indexed=S.open[S.kind[S.open] == 1], form="direct", n_hits=0, seams=["hit-0"])
    # C: launch groups
    ck = 1024
    tk_opts = [("use_tickets", 1), ("ticket_min_log2", 0), ("use_sub", 0)]
    sub_opts = [("use_sub", 1), ("sub_min_log2", 0), ("sub_words_log2", 5)]
    part = [("use_pregate", 2), ("use_partition", 1)]
    # (the partition form takes SoA tables only; what spills there depends on the coarse gate: these tables spread over 32 bins and
    # claim that nothing does, as in family F)
    for form, su, fo, entry in (("direct", "std", [], "device"), ("tickets", "tk-5", tk_opts, "device"), ("subs", "std", sub_opts, "device"), ("bins", "part-32", part, "device"),
                                ("direct", "std", [], "rows12"), ("tickets", "tk-5", tk_opts, "rows12"), ("subs", "std", sub_opts, "rows12")):
        pool_n = len(setup(su).rkmers)
        for n in (ck, ck + 1, 2 * ck - 1) + ((2 * ck + 2, 2 * ck + 3) if entry == "rows12" else ()):
            _add("C-%s-%s-n%d" % (form, entry, n), "C", "launch groups of 1,024 rows, the last one of %d" % ((n - 1) % ck + 1), su, fo + [("scan_chunk_log2", 10)],
                 tiled(np.arange(pool_n), n), entry=entry, form=form, seams=["chunks-" + form] + (["rows12-last-chunk-%d" % ((n - 1) % ck + 1)] if entry == "rows12" and (n - 1) % ck < 3 else []))
    for form, su, fo in (("direct", "std", []), ("tickets", "tk-5", tk_opts), ("subs", "std", sub_opts), ("bins", "part-32", part)):
        s5 = setup(su)
        hot = s5.open[np.isin(s5.kind[s5.open], [0, 2])]
        for first in ("hits", "none"):
            a, b = tiled(hot, ck), tiled(s5.closed, ck)
            _add("C-reset-%s-%s-first" % (form, first), "C", "the list lengths start from zero in every launch group: one group all hits, the other none", su,
                 fo + [("scan_chunk_log2", 10)], np.concatenate([a, b] if first == "hits" else [b, a]), form=form, seams=["chunk-counter-reset"])
    # D: the ticket form
    for P in (2, 3, 5, 7, 9, 256):
        su = "tk-%d" % P
        pool_n = len(setup(su).rkmers)
        for entry, off in (("device", 0), ("device", 1), ("rows12", 0)):
            _add("D-P%d-%s-o%d" % (P, entry, off), "D", "%d slices: nshare, the p += 8 stride%s" % (P, ", TK_MAXP" if P == 256 else ""), su, tk_opts, tiled(np.arange(pool_n), 5000 + P),
                 entry=entry, offset=off, form="tickets", nbins=P, seams=["slices-%d" % P] + (["unaligned-ticket-sort"] if off else []) + (["tickets-rows12"] if entry == "rows12" else []))
    T5 = setup("tk-5")
    slice_of = T5.word >> 1
    in0, rest = np.flatnonzero(slice_of == 0), np.flatnonzero(slice_of != 0)
    for d in (-1, 0, 1):
        _add("D-segcap%+d" % d, "D", "one segment filled to segcap%+d (scan_bin_cap 64)" % d, "tk-5", tk_opts + [("scan_bin_cap", 64)],
             np.concatenate([tiled(in0, 64 + d), tiled(rest, 40)]), form="tickets", spilled=max(d, 0), seams=["ticket-segcap"], exact_fill=(0, 64 + d))
    _add("D-one-slice", "D", "every row in one slice: natural overflow of the default segcap", "tk-5", tk_opts, tiled(in0, 6000), form="tickets", spilled_positive=True,
         seams=["ticket-natural-overflow"])
    t5hit = unblocked(T5, T5.open[(slice_of[T5.open] == 0) & np.isin(T5.kind[T5.open], [0, 2])])
    _add("D-all-pass", "D", "every ticket passes the gate: one workgroup's walk of four steps, a wave's stage at 1,536 then 2,048", "tk-5",
         tk_opts + [("ticket_gate_grid", 8), ("scan_bin_cap", 2048)], tiled(t5hit, 8 * 2048), form="tickets", all_hit=True, seams=["ticket-stage-full"])
    n3 = 8 * TKG_SPW * 1024 * 2 + 4096 + 77
    hole = lambda: np.arange(n3) // TK_TILE % 3 == 1            # every third tile's rows lie in other slices: slice 0 has empty segments between full ones
    o3 = lambda: np.where(hole(), tiled(rest, n3), tiled(in0, n3))
    _add("D-walks", "D", "ticket_gate_grid 8, more than 64 segments per workgroup: a second and a third walk, empty segments between full ones", "tk-5",
         tk_opts + [("ticket_gate_grid", 8), ("scan_bin_cap", TK_TILE)], o3, form="tickets", spilled=0, walks=True, seams=["ticket-second-walk"], large=True)
    nbig = 2048 * 2048 + 3 * 2048 + 5
    for entry, off in (("device", 0), ("device", 1), ("rows12", 0)):
        _add("D-second-tile-%s-o%d" % (entry, off), "D", "more than 2,048 tiles of 2,048 rows: workgroups sort a second tile (sh_hist parity, sh_pos carried)", "tk-5", tk_opts,
             lambda: tiled(np.arange(4096), nbig), entry=entry, offset=off, form="tickets", seams=["ticket-second-tile"], large=True)
    # E: the sub-slice form
    bin5 = (S.slot[every] >> U(S.shift + 6 + 5)).astype(np.int64)   # 8 bins of 32 words (the seeded rows)
    by_bin = [np.flatnonzero(bin5 == b) for b in range(8)]
    not0 = np.flatnonzero(bin5 != 0)
    fast, slow, fast_not0 = tiled(every, SB_TILE), tiled(by_bin[0], SB_TILE), tiled(not0, SB_TILE)
    slow3 = tiled(by_bin[3], SB_TILE)
    for entry in ("device", "rows12"):
        for grid in (1, 2):
            for seq, tiles in (("FFF", [fast, fast, fast]), ("FSF", [fast, slow, fast_not0]), ("SS", [slow, slow3]), ("FFFFF", [fast] * 5)):
                order = np.concatenate([np.concatenate([t] * grid) for t in tiles])           # each workgroup of the grid sees the sequence
                _add("E-%s-g%d-%s" % (seq, grid, entry), "E", "sub_grid %d, tiles %s: the deferred stores of scan_sub_sort_kernel around sh_slow" % (grid, seq), "std",
                     sub_opts + [("sub_grid", grid)], order, entry=entry, form="subs", nbins=8, modes=[seq] * grid, seams=["sub-deferred-" + seq] + (["subs-rows12"] if entry == "rows12" else []))
    for last in (1, SB_TILE - 1):
        order = tiled(every, 2 * SB_TILE + last)
        order[-1] = hit_rows[0]                                  # (the last tile's last row is one whose count must arrive)
        _add("E-last-tile-%d" % last, "E", "a last tile of %d rows" % last, "std", sub_opts + [("sub_grid", 1)], order, form="subs", nbins=8, last_row_hits=True,
             seams=["sub-last-tile"])
    for d in (-1, 0, 1):
        _add("E-segcap%+d" % d, "E", "a bin filled to segcap%+d (scan_bin_cap 512)" % d, "std", sub_opts + [("sub_grid", 1), ("scan_bin_cap", 512)],
             np.concatenate([tiled(by_bin[0], 512 + d), tiled(not0, 7 * 300)]), form="subs", nbins=8, spilled=max(d, 0), seams=["sub-segcap"], exact_fill=(0, 512 + d))
    for m in (639, 640, 641, 1281):
        _add("E-segment-%d" % m, "E", "a segment of %d tickets: %s" % (m, "one step" if m <= 640 else "rest()"), "std", sub_opts + [("sub_grid", 1)],
             np.concatenate([tiled(by_bin[0], m), tiled(not0, SB_TILE - m)]), form="subs", nbins=8, spilled=0, exact_fill=(0, m), seams=["sub-rest"] if m > 640 else ["sub-one-step"])
    for split in (1, 3, 64):
        _add("E-split-%d" % split, "E", "sub_split %d" % split, "std", sub_opts + [("sub_split", split)], tiled(every, 40000), form="subs", nbins=8, seams=["sub-split-%d" % split])
    _add("E-parts-8", "E", "8 bins on 8 or more tiles: parts = 8", "std", sub_opts + [("sub_grid", 9)], tiled(every, 9 * SB_TILE + 5), form="subs", nbins=8, parts=8, seams=["sub-parts-8"])
    _add("E-parts-1", "E", "256 single-word bins: parts = 1, nw = 1", "std", [("use_sub", 1), ("sub_min_log2", 0), ("sub_words_log2", 0)], tiled(every, 3 * SB_TILE + 5), form="subs",
         nbins=256, parts=1, seams=["sub-parts-1", "sub-single-word"])
    _add("E-partial-last", "E", "32 bins of 8 words over 255 gate words: the last sub-slice holds 7, and rows sit in the gate's last word", "sub-partial",
         [("use_sub", 1), ("sub_min_log2", 0), ("sub_words_log2", 3)], tiled(np.arange(4096), 20000), form="subs", nbins=32, last_word=254, seams=["sub-partial-last"])
    _add("E-1024-bins", "E", "1,024 bins: the most the form takes", "sub-1024", [("use_sub", 1), ("sub_min_log2", 0), ("sub_words_log2", 0)], tiled(np.arange(8192), 40000),
         form="subs", nbins=1024, seams=["sub-1024-bins"])
    for m in (1023, 1024, 1025):
        _add("E-spill-%d" % m, "E", "a spill list of %d tickets" % m, "std", sub_opts + [("sub_grid", 1), ("scan_bin_cap", 16)], tiled(by_bin[2], 16 + m), form="subs", nbins=8,
             spilled=m, seams=["sub-spill-list"])
    for lazy in (0, 1):
        _add("E-lazy-%d" % lazy, "E", "lazy_vectors %d with the records' copies live" % lazy, "std", sub_opts + [("use_record_counters", 2), ("lazy_vectors", lazy)], tiled(every, 40000),
             form="subs", nbins=8, seams=["sub-lazy-%d" % lazy])
    _add("E-sub-grid-clamp", "E", "sub_grid 4096 is clamped to SB_MAXB = 1,024: more tiles than that on 512 single-word bins (parts = 1), a wave's fills one per lane", "sub-1024",
         [("use_sub", 1), ("sub_min_log2", 0), ("sub_words_log2", 1), ("sub_grid", 4096)], lambda: tiled(np.arange(8192), 1026 * SB_TILE + 3), form="subs", nbins=512, parts=1, nseg=1024,
         seams=["sub-grid-clamp"], large=True)
    # F: the partition form
    for rows in (2, 4):
        for ring in (64, 128, 256):
            su = "part-32" if ring == 64 else "part-2"
            _add("F-r%d-ring%d" % (rows, ring), "F", "scan_bin_kernel<%d>, ring %d, %s slices" % (rows, ring, su[5:]), su, part + [("scan_bin_rows", rows), ("scan_bin_ring", ring)],
                 tiled(np.arange(4096), 30011), form="bins", nbins=int(su[5:]), seams=["bin-rows-%d" % rows, "bin-ring-%d" % ring, "bin-P-" + su[5:]])
    F = setup("part-32")
    one = F.open[(F.word[F.open] >> 3) == 4]
    _add("F-one-bin", "F", "every survivor in one bin: lanes deferred, the `again` loop turns", "part-32", part, np.concatenate([tiled(one, 9000), tiled(F.closed, 1000)]), form="bins",
         nbins=32, spilled_positive=True, seams=["bin-one-bin"])
    _add("F-second-iteration", "F", "more than 2,048 tiles of 1,024 rows: a workgroup of scan_bin_kernel<4> takes a second iteration", "part-32", part + [("scan_bin_rows", 4)],
         lambda: tiled(np.arange(4096), 2048 * 1024 + 3 * 1024 + 5), form="bins", nbins=32, seams=["bin-second-iteration"], large=True)
    # G: slots and keys, through the direct, ticket and sub-slice forms
    G = setup("slots")
    g_rows = np.concatenate([G.slot_rows[s] for s in SLOT_TARGETS] + [G.twins])
    g_forms = (("direct", []), ("tickets", [("pregate_log2", 8), ("gate_log2", 30)] + tk_opts), ("subs", [("use_sub", 1), ("sub_min_log2", 0), ("sub_words_log2", 0)]))
    for form, fo in g_forms:
        for ordered in (0, 1):
            _add("G-slots-%s-ord%d" % (form, ordered), "G", "rows at slot 0, size - 1, both sides of every gate word, slice and sub-slice, three adjacent slots; twins of one centre "
                 "k-mer in and out of context_bf; map_ordered %d" % ordered, "slots", fo + [("map_ordered", ordered), ("use_record_counters", 2)], tiled(g_rows, 3 * len(g_rows) + 1), indexed=g_rows,
                 form=form, nbins={"direct": 0, "tickets": 2, "subs": 4}[form], seams=["slot-edges", "context-twins", "key-and-bit"] + (["shared-record"] if ordered else []))
    for form, su, fo, entry in (("direct", "k34-44", [], "device"), ("tickets", "k34-44-tk", tk_opts, "device"), ("subs", "k34-44", sub_opts, "rows12")):
        E34 = setup(su)
        _add("G-palindrome-%s" % form, "G", "k = 34: centre k-mers equal to their own reverse complement", su, fo, tiled(np.concatenate([E34.pal, np.arange(500)]), 3000),
             entry=entry, form=form, seams=["palindrome"])
    _add("G-refscan-context", "G", "context_bf filled by the reference scan, not by inserts", "std-refscan", [], tiled(every, 9000), form="direct", seams=["refscan-context"])
    # H: counters.  The two bf rows of H_PAIR are entries 0 and 1 of one record, the two 16-bit halves of one word.  One of them is
    # taken through 2^16 while the other is left at 7 -- which must not change: not by a carry out of the low half, not by an add
    # sent to the wrong entry -- and then the other way round (w0, w1: which of the two is entry 0 is the build kernel's business).
    hrow, hrow2, hmap = S.h_pair
    h = S.h
    others = S.open[~np.isin(S.slot[S.open], S.slot[[hrow, hrow2, hmap]])]
    bf_tables = {"single-65535": ([65535], 65535), "single-65536": ([65536], 0), "single-65537": ([65537], 1),
                 "copies-65535": ([1] * 100000 + [31071], 65535), "copies-65536": ([1] * 100000 + [31072], 0), "copies-65537": ([1] * 100000 + [31073], 1),
                 "zero-and-max": ([0, 0xFFFFFFFF, 0xFFFFFFFF], 65534)}
    map_tables = {"map-2^31": ([(1 << 31) - 1, 1], -(1 << 31)), "map-2^32": ([1 << 31, 1 << 31, 1], 1), "map-max-twice": ([0xFFFFFFFF, 0xFFFFFFFF, 0], -2)}
    h_tables = {}
    for tname, (counts, want) in bf_tables.items():
        for w in (0, 1):
            h_tables["%s-w%d" % (tname, w)] = ([h["bf", c][w] for c in counts] + [h["bf", 7][1 - w], h["map", 0][0]],
                                             [("bf", (hrow, hrow2)[w], want), ("bf", (hrow, hrow2)[1 - w], 7)])
    for tname, (counts, want) in map_tables.items():
        h_tables[tname] = ([h["map", c][0] for c in counts], [("map", hmap, want)])
    # 100,000 rows (200,000 when measured) on one record: every thread in flight retries its compare-and-swap against every other
    # one (rec_add_bf), so the time grows with the SQUARE of what is in flight -- measured 58 s per case with the default grids
    # (262,144 threads), well under a second with 2,048.  A table holds each k-mer once, so nothing real comes near; the cases keep
    # their 100,000 copies and bound the grid.
    crowd = [("hits_grid", 8), ("probe_grid", 4)]
    for tname, (rows, counters) in h_tables.items():
        for rc in (0, 1, 2):
            for form, fo in (("direct", []), ("subs", sub_opts + [("lazy_vectors", 1)])):
                # beside the counters under test every other indexed pool row is scanned once: each neighbour holds its own known count
                _add("H-%s-rc%d-%s" % (tname, rc, form), "H", "a counter taken through a power of two (%s), its neighbour in the record held at 7; use_record_counters %d" % (tname, rc), "std",
                     fo + [("use_record_counters", rc), ("map_ordered", 1)] + crowd * (len(rows) > 1000), np.concatenate([np.asarray(rows), others]), form=form,
                     counter=counters, seams=["counter-wrap-" + tname.split("-")[0], "record-counters-%d" % rc] + (["contention"] if len(rows) > 1000 else []))


_build()

# every seam the suite is there for, and (filled by the CPU file's completeness test) the cases that name it
SEAMS = ["rows-1", "rows-2", "rows-4", "variant-0", "variant-2", "unaligned-direct", "partial-tile", "carry-over", "multi-iteration-direct", "gated-carry",
         "rows12-nmod4-0", "rows12-nmod4-1", "rows12-nmod4-2", "rows12-nmod4-3", "rows12-maxcount", "rows12-padding",
         "probe-carry", "hit-entries-0", "hit-entries-1", "open-0", "hit-0",
         "chunks-direct", "chunks-tickets", "chunks-subs", "chunks-bins", "rows12-last-chunk-1", "rows12-last-chunk-2", "rows12-last-chunk-3", "chunk-counter-reset",
         "slices-2", "slices-3", "slices-5", "slices-7", "slices-9", "slices-256", "unaligned-ticket-sort", "tickets-rows12", "ticket-segcap", "ticket-natural-overflow",
         "ticket-stage-full", "ticket-second-walk", "ticket-second-tile",
         "sub-deferred-FFF", "sub-deferred-FSF", "sub-deferred-SS", "sub-deferred-FFFFF", "subs-rows12", "sub-last-tile", "sub-segcap", "sub-one-step", "sub-rest",
         "sub-split-1", "sub-split-3", "sub-split-64", "sub-parts-1", "sub-parts-8", "sub-single-word", "sub-partial-last", "sub-1024-bins", "sub-spill-list",
         "sub-lazy-0", "sub-lazy-1", "sub-grid-clamp",
         "bin-rows-2", "bin-rows-4", "bin-ring-64", "bin-ring-128", "bin-ring-256", "bin-P-2", "bin-P-32", "bin-one-bin", "bin-second-iteration",
         "slot-edges", "context-twins", "key-and-bit", "shared-record", "palindrome", "refscan-context",
         "counter-wrap-single", "counter-wrap-copies", "counter-wrap-map", "counter-wrap-zero", "record-counters-0", "record-counters-1", "record-counters-2", "contention"]


def case_ids():
    return list(_CASES)


def case(name):
    return _CASES[name]


# ---- a case's index, table and expected result --------------------------------------------------------------------------------
def index_of(c):
    """(bf k-mers, map k-mers, context ref_k-mers, genome or None) as byte strings"""
    s = setup(c.setup)
    bf, mp, cx = s.index_lists(c.indexed)
    genome = None
    if s.ctx == "refscan":                                      # the blocked rows' ref_k-mers back to back: every one of them is a window whose centre hits bf
        genome = b"".join(s.rkmers[i] for i in cx)
        cx = []
    return [s.centres[i] for i in bf], [s.centres[i] for i in mp], [s.rkmers[i] for i in cx], genome


def oracle_index(c):
    s = setup(c.setup)
    bf, mp, cx, genome = index_of(c)
    obf, octx, omap = ocapi.BF(s.bits), ocapi.BF(s.bits), ocapi.KMAP()
    for km in bf:
        obf.add_key(km)
    for km in mp:
        omap.add_key(km)
    obf.switch_mode()
    if genome is not None:
        ocapi.ref_scan(obf, octx, genome, s.k, s.ref_k)
    for km in cx:
        octx.add_key(km)
    octx.switch_mode()
    return obf, octx, omap


def counts_of(c):
    """the pool's counts as this case's table carries them"""
    s = setup(c.setup)
    cnt = s.cnt.copy()
    if "maxcount" in c.claims:
        cnt[:] = c.claims["maxcount"]
    return cnt


def table(c):
    """(hi, lo, cnt) of every table row"""
    s = setup(c.setup)
    return s.hi[c.order], s.lo[c.order], counts_of(c)[c.order]


def expected(c):
    """(obf, octx, omap) after the scan, by the multiplicity identity: one oracle scan of the pool rows the table holds"""
    s = setup(c.setup)
    obf, octx, omap = oracle_index(c)
    mult = np.bincount(c.order, minlength=len(s.rkmers)).astype(np.uint64)
    used = np.flatnonzero(mult)
    cnt = ((counts_of(c).astype(np.uint64)[used] * mult[used]) & U(0xFFFFFFFF)).astype(np.uint32)
    ocapi.kmc_scan_packed(octx, obf, omap, s.hi[used], s.lo[used], cnt, s.k, s.ref_k)
    return obf, octx, omap


def bits_set(words, slots):
    return ((words[(slots >> U(6)).astype(np.int64)] >> (slots & U(63))) & U(1)).astype(bool)


def model(c, obf_words, cus=CUS):
    """what the device must report: form, nbins, spilled tickets of the last launch group (None: not claimed), n_hits of the
    whole call, open rows of the last launch group"""
    s = setup(c.setup)
    n = len(c.order)
    p = plan(s.bits, dict(s.options() + list(c.opts)), n, c.entry.startswith("rows12"), cus)
    slots = s.slot[c.order]
    r0, nr = last_chunk(p, n)
    hit = bits_set(obf_words, slots)
    indexed = np.zeros(len(s.rkmers), dtype=bool)
    bf, mp, _ = s.index_lists(c.indexed)
    indexed[bf] = indexed[mp] = True
    # open: the row shares its slot with an indexed row (the gate's bits are a function of the slot); closed: its gate word holds
    # no indexed row; else either.  With the gate off (use_summary 0) every row is listed.
    word = (slots >> U(s.shift + 6)).astype(np.int64)
    sure = np.isin(slots, s.slot[indexed])
    maybe = np.isin(word, s.word[indexed]) & ~sure
    if not dict(c.opts).get("use_summary", 1):
        sure, maybe = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
    lo = int(sure[r0:].sum())
    m = dict(form=p["form"], nbins=p["nbins"], n_hits=int(hit.sum()), n_open=(lo, lo + int(maybe[r0:].sum())), plan=p, spilled=None)
    if p["form"] in ("tickets", "subs"):
        m["spilled"] = spilled(p, slots[r0:])
    return m
