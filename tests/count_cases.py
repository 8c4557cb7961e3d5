"""Directed cases for the four cell counters behind `call --cohort`: mg_pack_dosage and mg_pair_counts (--pairs), mg_sample_counts
(--sample-stats), mg_site_counts (--site-tags) and mg_site_geno_counts (--site-stats).  No GPU and no HIP here:
tests/test_count_cases_cpu.py proves on any machine that every case holds the seams it claims and that its written-down expectation
is what the numpy restatements of the existing test files make of its inputs; tests/test_gpu_count_edges.py hands the same arrays to
the device.

A seam is a place where a cell meets an edge of a kernel: the chunk and the run of pair_count_kernel's word loop, a tile of its pairs,
the carry of a 64-bit counter, a lane that stores a word of pack_dosage_kernel, a step and a run of sample_count_kernel, a round of
SITE_BINS in the two site kernels.  A case is built by putting cells down one at a time, and its expected output is a tally of what was
put where -- never a model run over the finished arrays:

  pairs     every row (plane, dosage) of an operand is a set of (word, bit) positions or ALL ONES; a placement (i, da, j, db, word, bit)
            owns its position, so the rows meet exactly where a placement, a full word or two all-ones rows make them meet
  packing   the background has no class (allele indexes -1); a directed cell states its class, or None
  samples   the background is a called hom-ref cell of GQ 50 and status 0, so RECORDS = CALLED = HOM_REF = n; a directed cell replaces
            one background cell and states every slot it adds to
  sites     a directed cell states the alleles mg_site_counts counts for it and the homozygote or heterozygote mg_site_geno_counts makes
            of it; one table of cells goes through both kernels

The plans that decide where a run ends are the restatement of tests/test_count_plan_cpu.py, which that file holds against the
library's header."""
import numpy as np

from test_count_plan_cpu import pair_plan, pair_tiles, sample_plan
from test_sample_stats_cpu import SLOTS, SS

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
U32_MAX = (1 << 32) - 1
M64 = (1 << 64) - 1
ONES = np.uint64(M64)
EDGE_PLANES = (0, 15, 16, 17, 31, 32, 47, 48, 63)           # both sides of every tile of PAIR_TILE = 16 planes
PAIR_TILE, PAIR_CHUNK = 16, 32                              # pair_kernels.h, count_plan.h (a test's copy)
SITE_BINS, SITE_BALLOT_MAX = 128, 8                         # site_tags_kernels.h (a test's copy)
ALL_ONES = "all ones"


# ==== pairs, counting ================================================================================================================

class PairCase:
    kind = "pair"

    def __init__(self, name, n_a, n_b, n_words, symmetric, cut):
        assert not symmetric or n_a == n_b
        self.name, self.n_a, self.n_b, self.n_words, self.symmetric, self.cut = name, n_a, n_b, n_words, symmetric, cut
        self.seams = []
        self.rows = {"a": {}, "b": {}}                      # (plane, dosage) -> set of (word, bit), or ALL_ONES
        self.owned = set()                                  # positions a placement, a decoy or a full word has taken
        self.placements, self.decoys, self.ones, self.full_words = [], [], [], []
        self.start = None                                   # the table an accumulating call starts from (None: zeros)
        assert 0 < cut < n_words

    # -- construction
    def _row(self, op, plane, d):
        assert 0 <= plane < (self.n_a if op == "a" else self.n_b) and 0 <= d < 3
        row = self.rows["a" if self.symmetric else op].setdefault((plane, d), set())
        assert row is not ALL_ONES, "a row of all ones takes no cells"
        return row

    def _own(self, word, bit):
        assert 0 <= word < self.n_words and 0 <= bit < 64 and (word, bit) not in self.owned, (word, bit)
        self.owned.add((word, bit))

    def place(self, i, da, j, db, word, bit):
        """one bit that row (i, da) of A and row (j, db) of B share"""
        self._own(word, bit)
        self._row("a", i, da).add((word, bit))
        self._row("b", j, db).add((word, bit))
        self.placements.append((i, da, j, db, word, bit))

    def decoy(self, j, db, word, bit):
        """one bit of row (j, db) of B that no row of A shares (B is A: that no other row shares)"""
        self._own(word, bit)
        self._row("b", j, db).add((word, bit))
        self.decoys.append((j, db, word, bit))

    def full_word(self, i, da, j, db, word):
        for bit in range(64):
            self._own(word, bit)
            self._row("a", i, da).add((word, bit))
            self._row("b", j, db).add((word, bit))
        self.full_words.append((i, da, j, db, word))

    def ones_pair(self, i, da, j, db):
        for op, key in (("a", (i, da)), ("b", (j, db))):
            rows = self.rows["a" if self.symmetric else op]
            assert not rows.get(key), "the row already holds cells"
            rows[key] = ALL_ONES
        self.ones.append((i, da, j, db))

    def is_ones(self, op, plane, d):
        return self.rows["a" if self.symmetric else op].get((plane, d)) is ALL_ONES

    # -- what the construction makes
    def tiles(self):
        return pair_tiles(self.n_a, None if self.symmetric else self.n_b)

    def plan(self):
        return pair_plan(self.n_words, self.tiles())

    def planes(self):
        """-> (A, B) uint64 [n, 3, n_words]; B is None in the symmetric form"""
        def dense(rows, n):
            p = np.zeros((n, 3, self.n_words), dtype=np.uint64)
            for (plane, d), row in rows.items():
                if row is ALL_ONES:
                    p[plane, d] = ONES
                else:
                    for word, bit in row:
                        p[plane, d, word] |= np.uint64(1 << bit)
            return p
        return dense(self.rows["a"], self.n_a), None if self.symmetric else dense(self.rows["b"], self.n_b)

    def expected(self):
        """-> uint64 [n_a, n_b, 3, 3]: rows meet where they were made to meet"""
        a = self.rows["a"]
        b = a if self.symmetric else self.rows["b"]
        out = np.zeros((self.n_a, self.n_b, 3, 3), dtype=np.uint64)
        for (i, da), x in a.items():
            for (j, db), y in b.items():
                if x is ALL_ONES and y is ALL_ONES:
                    c = 64 * self.n_words
                elif x is ALL_ONES:
                    c = len(y)
                elif y is ALL_ONES:
                    c = len(x)
                else:
                    c = len(x & y)
                out[i, j, da, db] = c
        return out

    def start_table(self):
        return np.zeros((self.n_a, self.n_b, 3, 3), dtype=np.uint64) if self.start is None else self.start.copy()


TRIP_WORDS = ("0", "31", "32", "33", "run-1", "run", "run+31", "run+32", "last", "last-run-first", "last-run-last")


def trip_word(name, n_words, run, n_runs):
    return {"0": 0, "31": 31, "32": 32, "33": 33, "run-1": run - 1, "run": run, "run+31": run + 31, "run+32": run + 32, "last": n_words - 1,
            "last-run-first": (n_runs - 1) * run, "last-run-last": n_words - 1}[name]


def _form(symmetric):
    return "sym" if symmetric else "exp"


def _trip_case(n, n_words, symmetric):
    """one-hot placements at every seam word of the plan's runs, a decoy on both sides of each, one pair of all-ones rows"""
    run, n_runs = pair_plan(n_words, pair_tiles(n, None if symmetric else n))
    c = PairCase("pair-trips-%dx%d-%dw-%s" % (n, n, n_words, _form(symmetric)), n, n, n_words, symmetric, cut=run + 1)
    planes = [p for p in EDGE_PLANES if p < n] if n > 2 else [0, 1]
    ones_a, ones_b = (1 % n, 1), (n - 1, 2)
    c.ones_pair(*ones_a, *ones_b)
    taken = {ones_a, ones_b}
    words = sorted({trip_word(w, n_words, run, n_runs) for w in TRIP_WORDS})
    assert words[0] == 0 and words[-1] == n_words - 1
    for k, word in enumerate(words):
        i, j = planes[k % len(planes)], planes[(2 * k + 1) % len(planes)]
        da, db = k % 3, (k // 3 + k) % 3
        while (i, da) in taken:
            da = (da + 1) % 3
        while (j, db) in taken:
            db = (db + 1) % 3
        if n == 2:                                            # (six rows, two of them all ones: two pairs of rows take turns, so that
            i, da, j, db = ((0, 0, 0, 1), (0, 2, 1, 0))[k % 2]  # each keeps a row it never meets, for its decoys)
        bit = (11 * k + 5) % 64                               # (fewer than 64 placements: every one a bit of its own)
        c.place(i, da, j, db, word, bit)
    # a decoy on either side of every placement: the placement's bit, one word off, in a row of B that row (i, da) of A never meets --
    # so a word of B read one off against A turns an entry that must be 0 into 1 (and the placement's own entry into 0)
    meets = set()
    for i, da, j, db, word, bit in c.placements:
        meets |= {(i, da, j, db)} | ({(j, db, i, da), (i, da, i, da), (j, db, j, db)} if symmetric else set())
    ones_b = {ones_a, ones_b} if symmetric else {ones_b}
    for i, da, j, db, word, bit in list(c.placements):
        rows = [(j, d) for d in range(3) if d != db] + [(p, d) for p in planes if p != j for d in range(3)]
        row = next(r for r in rows if r not in ones_b and (i, da) + r not in meets and not (symmetric and r == (i, da)))
        for near in (word - 1, word + 1):
            if 0 <= near < n_words:
                c.decoy(*row, near, bit)
    f = "/" + _form(symmetric)
    c.seams += ["trips-%d" % (run // PAIR_CHUNK) + f, "tiles-%d" % c.tiles() + f, "ones-pair" + f, "decoy-before" + f, "decoy-after" + f]
    c.seams += ["word-" + w + f for w in TRIP_WORDS if w in ("0", "31", "last") or n_runs > 1]
    last = n_words - (n_runs - 1) * run
    if n_runs > 1 and last == 1:
        c.seams.append("last-run-1-word" + f)
    if n_runs > 1 and last == 33:
        c.seams.append("last-run-33-words" + f)
    if c.tiles() == 1 and n_runs >= 1000:
        c.seams.append("word-axis-only" + f)
    return c


# 17 planes are 3 tiles in the symmetric form: 682 runs at most, so 682 chunks and a word are runs of two chunks, the last of one word
N_WORDS_17 = (2048 // 3) * PAIR_CHUNK + 1
TRIP_SHAPES = ((64, 4097), (64, 8193), (64, 6529), (2, 65537), (2, 131073), (17, N_WORDS_17))


def _tile_case(n_a, n_b):
    """every pair of edge planes holds all nine entries, entry (da, db) of pair (i, j) a count of its own"""
    symmetric = n_b is None
    name = "pair-square-%d" % n_a if symmetric else "pair-block-%dx%d" % (n_a, n_b)
    c = PairCase(name, n_a, n_a if symmetric else n_b, 256, symmetric, cut=100)
    pa = [p for p in EDGE_PLANES if p < n_a]
    pb = pa if symmetric else [p for p in EDGE_PLANES if p < n_b]
    at = 0
    for ki, i in enumerate(pa):
        for kj, j in enumerate(pb):
            if symmetric and i > j:
                continue                                      # (the pair (j, i) is this pair's mirror)
            for da in range(3):
                for db in range(3):
                    if symmetric and i == j and da > db:
                        continue                              # (the same two rows)
                    for _ in range(1 + 3 * da + db + 9 * ((ki + 2 * kj) % 3)):
                        c.place(i, da, j, db, at // 64, (at % 64) * 37 % 64)
                        at += 1
    assert at <= 64 * c.n_words
    c.seams.append(("square-%d" % n_a) if symmetric else "block-%dx%d" % (n_a, n_b))
    c.seams += ["plane-%d-a" % p for p in pa] + ["plane-%d-b" % p for p in pb]
    diag = any(i // PAIR_TILE == j // PAIR_TILE for i in pa for j in pb)
    off = any(i // PAIR_TILE != j // PAIR_TILE for i in pa for j in pb)
    for da in range(3):
        for db in range(3):
            c.seams += ["entry-%d%d-diagonal" % (da, db)] * diag + ["entry-%d%d-off" % (da, db)] * off
    if symmetric and off:
        c.seams.append("mirror-transposed")
    return c


TILE_BLOCKS = ((17, 33), (33, 17), (64, 17), (16, 64), (1, 64))
TILE_SQUARES = (17, 32, 33, 64)
CARRY_STARTS = (("2^32-1", (1 << 32) - 1), ("2^32", 1 << 32), ("2^63-1", (1 << 63) - 1))
CARRY_ADDS = (("1", 1), ("64", 64), ("64n", 64 * 33))


def _carry_case(symmetric):
    """17 x 17 planes, 33 words: entries that receive 1, 64 and 64 n_words on top of 2^32 - 1, 2^32 and 2^63 - 1, every other entry on
    top of a number of its own"""
    n, n_words = 17, 33
    c = PairCase("pair-carry-" + _form(symmetric), n, n, n_words, symmetric, cut=32)
    receives = {"1": [(0, 0, 16, 1), (16, 2, 1, 0), (2, 1, 2, 1)], "64": [(3, 0, 4, 1), (16, 1, 3, 2), (5, 2, 16, 0)],
                "64n": [(6, 0, 9, 2), (7, 1, 10, 0), (8, 2, 11, 1)]}
    for k, (i, da, j, db) in enumerate(receives["1"]):
        c.place(i, da, j, db, (3, 31, 31)[k], (0, 63, 17)[k])
    for k, (i, da, j, db) in enumerate(receives["64"]):
        c.full_word(i, da, j, db, (0, 30, 32)[k])
    for i, da, j, db in receives["64n"]:
        c.ones_pair(i, da, j, db)
    start = (1000 + np.arange(n * n * 9, dtype=np.uint64)).reshape(n, n, 3, 3)     # asymmetric: every entry a number of its own
    for add, _ in CARRY_ADDS:
        for (_, s), (i, da, j, db) in zip(CARRY_STARTS, receives[add]):
            start[i, j, da, db] = s
    c.start = start
    f = "/" + _form(symmetric)
    c.seams += ["carry-%s-plus-%s" % (s, a) + f for s, _ in CARRY_STARTS for a, _ in CARRY_ADDS] + ["untouched-asymmetric" + f]
    return c


SMALL_WORDS = (31, 32, 33, 63, 64, 65)


def _small_case(n_words, symmetric):
    c = PairCase("pair-small-%dw-%s" % (n_words, _form(symmetric)), 2, 2, n_words, symmetric, cut=32 if n_words > 32 else n_words - 1)
    c.place(0, 0, 0, 0, n_words - 1, 0)
    c.place(1, 2, 1, 1, n_words - 1, 63)
    c.ones_pair(0, 2, 0, 1)
    f = "/" + _form(symmetric)
    c.seams += ["words-%d" % n_words + f, "last-word-bit-0" + f, "last-word-bit-63" + f, "ones-pair" + f]
    return c


def pair_cases():
    out = [_trip_case(n, w, s) for n, w in TRIP_SHAPES for s in (True, False)]
    out += [_tile_case(a, b) for a, b in TILE_BLOCKS] + [_tile_case(n, None) for n in TILE_SQUARES]
    out += [_carry_case(s) for s in (True, False)]
    out += [_small_case(w, s) for w in SMALL_WORDS for s in (True, False)]
    return out


def _required_pair():
    req = []
    for f in ("/sym", "/exp"):
        req += ["trips-1/sym"] * (f == "/sym") + ["trips-2" + f, "trips-3" + f, "last-run-1-word" + f, "last-run-33-words" + f, "word-axis-only" + f, "tiles-1" + f, "ones-pair" + f,
                "decoy-before" + f, "decoy-after" + f, "untouched-asymmetric" + f, "last-word-bit-0" + f, "last-word-bit-63" + f]
        req += ["word-" + w + f for w in TRIP_WORDS]
        req += ["carry-%s-plus-%s" % (s, a) + f for s, _ in CARRY_STARTS for a, _ in CARRY_ADDS]
        req += ["words-%d" % w + f for w in SMALL_WORDS]
    req += ["tiles-16/exp", "tiles-10/sym", "tiles-4/exp", "tiles-3/sym", "mirror-transposed"]
    req += ["block-%dx%d" % b for b in TILE_BLOCKS] + ["square-%d" % n for n in TILE_SQUARES]
    req += ["plane-%d-%s" % (p, op) for p in EDGE_PLANES for op in "ab"]
    req += ["entry-%d%d-%s" % (da, db, where) for da in range(3) for db in range(3) for where in ("diagonal", "off")]
    return req


def shifted_entries(c, a, b, want, placement, step):
    """the entries (i, jd, da, dd) that must be 0 and would read 1 or more if row (i, da) of A at the placement's word met the words of
    B one `step` off; b is a in the symmetric form"""
    i, da, j, db, word, bit = placement
    near = word + step
    if not 0 <= near < c.n_words:
        return []
    x = a[i, da, word]
    return [(i, jd, da, dd) for jd in range(b.shape[0]) for dd in range(3)
            if not c.is_ones("b", jd, dd) and int(x & b[jd, dd, near]) and int(want[i, jd, da, dd]) == 0]


def pair_holds(c, seam, a, b, want):
    """is `seam` true of the case's inputs: the planes (a, b) it hands over, the plan of its shape, its expected table `want`"""
    b = a if b is None else b
    base, _, form = seam.partition("/")
    if form and (form == "sym") != c.symmetric:
        return False
    run, n_runs = c.plan()
    bit_of = lambda p, plane, d, word, bit: bool((int(p[plane, d, word]) >> bit) & 1)
    met = lambda i, da, j, db, word, bit: bit_of(a, i, da, word, bit) and bit_of(b, j, db, word, bit)
    if base.startswith("trips-"):
        return n_runs > 1 and run == int(base[6:]) * PAIR_CHUNK
    if base == "last-run-1-word":
        return n_runs > 1 and c.n_words - (n_runs - 1) * run == 1
    if base == "last-run-33-words":
        return n_runs > 1 and c.n_words - (n_runs - 1) * run == 33
    if base.startswith("tiles-"):
        return c.tiles() == int(base[6:])
    if base == "word-axis-only":
        return c.tiles() == 1 and n_runs >= 1000
    if base.startswith("word-"):
        name = base[5:]
        if name.startswith(("run", "last-run")) and n_runs < 2:
            return False
        word = trip_word(name, c.n_words, run, n_runs)
        return any(w == word and met(i, da, j, db, w, bit) and int(want[i, j, da, db]) >= 1 for i, da, j, db, w, bit in c.placements)
    if base in ("decoy-before", "decoy-after"):
        # proved from the arrays: at some placement, the word of B one off meets the placement's word of A in an entry that must be 0
        step = -1 if base == "decoy-before" else 1
        return any(shifted_entries(c, a, b, want, pl, step) for pl in c.placements)
    if base == "ones-pair":
        return any((a[i, da] == ONES).all() and (b[j, db] == ONES).all() and int(want[i, j, da, db]) == 64 * c.n_words for i, da, j, db in c.ones)
    if base.startswith("block-"):
        return not c.symmetric and base == "block-%dx%d" % (c.n_a, c.n_b)
    if base.startswith("square-"):
        return c.symmetric and base == "square-%d" % c.n_a
    if base.startswith("plane-"):
        _, p, op = base.split("-")
        return any((i if op == "a" else j) == int(p) and met(i, da, j, db, w, bit) for i, da, j, db, w, bit in c.placements)
    if base.startswith("entry-"):
        _, e, where = base.split("-")
        same = where == "diagonal"
        return any((da, db) == (int(e[0]), int(e[1])) and (i // PAIR_TILE == j // PAIR_TILE) == same and met(i, da, j, db, w, bit) and int(want[i, j, da, db])
                   for i, da, j, db, w, bit in c.placements)
    if base == "mirror-transposed":
        return c.symmetric and any(i // PAIR_TILE != j // PAIR_TILE and da != db and int(want[i, j, da, db]) != int(want[i, j, db, da]) and
                                   int(want[j, i, db, da]) == int(want[i, j, da, db]) for i, da, j, db, w, bit in c.placements)
    if base.startswith("carry-"):
        s, _, add = base[6:].partition("-plus-")
        s, add = dict(CARRY_STARTS)[s], dict(CARRY_ADDS)[add]
        return c.start is not None and bool(((c.start == np.uint64(s)) & (want == np.uint64(add))).any())
    if base == "untouched-asymmetric":
        return c.start is not None and not np.array_equal(c.start, c.start.transpose(1, 0, 3, 2)) and bool((want == 0).any()) and \
            len(np.unique(c.start[want == 0])) == int((want == 0).sum())
    if base.startswith("words-"):
        return c.n_words == int(base[6:]) and c.n_a == 2
    if base in ("last-word-bit-0", "last-word-bit-63"):
        bit = int(base.rsplit("-", 1)[1])
        return any(w == c.n_words - 1 and k == bit and int(a[i, da, w]) == 1 << bit and int(b[j, db, w]) == 1 << bit for i, da, j, db, w, k in c.placements)
    raise KeyError(seam)


class PackToCount:
    """cells that pack to the planes of a trip shape -- 2 planes x 65,537 words, one tile, the last word one record -- and the table
    they count to.  The background is 0/0 on both planes; a directed record states the dosage of each plane, or None for a cell
    without a class"""
    n_words = 65537
    n = 64 * n_words - 63

    def __init__(self):
        self.run, self.n_runs = pair_plan(self.n_words, 1)
        self.g1, self.g2 = np.zeros((2, self.n), dtype=np.int32), np.zeros((2, self.n), dtype=np.int32)
        self.directed = {}                                  # record -> (dosage of plane 0, dosage of plane 1)
        cells = {0: (0, 0), 1: (0, 1), 2: (1, 1), None: (-1, 0)}
        combos = [(da, db) for da in (0, 1, 2) for db in (0, 1, 2)] + [(None, 2), (1, None)]
        words = sorted({trip_word(w, self.n_words, self.run, self.n_runs) for w in TRIP_WORDS})
        for k, word in enumerate(words):
            record = 64 * word + (0 if word == self.n_words - 1 else (11 * k + 5) % 64)
            ds = combos[(k + 4) % len(combos)]                # (k = 0 is not the background's own (0, 0))
            for plane, d in enumerate(ds):
                self.g1[plane, record], self.g2[plane, record] = cells[d]
            self.directed[record] = ds

    def vao(self):
        return np.arange(0, 2 * self.n + 1, 2, dtype=np.uint32)

    def expected(self):
        out = np.zeros((2, 2, 3, 3), dtype=np.uint64)
        out[:, :, 0, 0] = self.n - len(self.directed)
        for ds in self.directed.values():
            for p in range(2):
                for q in range(2):
                    if ds[p] is not None and ds[q] is not None:
                        out[p, q, ds[p], ds[q]] += np.uint64(1)
        return out


_PACK_TO_COUNT = None


def pack_to_count():
    global _PACK_TO_COUNT
    if _PACK_TO_COUNT is None:
        _PACK_TO_COUNT = PackToCount()
    return _PACK_TO_COUNT


# ==== pairs, packing ==================================================================================================================

class CellCase:
    """cells [planes, n] over records of A alleles each; the arrays a kernel does not read stay None"""

    def __init__(self, name, planes, n, alleles, g, gq, haploid=False, min_gq=None):
        self.name, self.planes, self.n, self.haploid, self.min_gq = name, planes, n, haploid, min_gq
        self.seams = []
        self.A = np.full(n, alleles, dtype=np.int64)
        self.g1 = np.full((planes, n), g, dtype=np.int32)
        self.g2 = np.full((planes, n), g, dtype=np.int32)
        self.gq = np.full((planes, n), gq, dtype=np.int32)
        self.directed = {}                                  # (plane, record) -> what the cell was put there as

    def put(self, plane, record, g1, g2, gq=None, what=None):
        assert (plane, record) not in self.directed and 0 <= plane < self.planes and 0 <= record < self.n
        self.g1[plane, record], self.g2[plane, record] = g1, g2
        if gq is not None:
            self.gq[plane, record] = gq
        self.directed[(plane, record)] = what

    def vao(self):
        v = np.zeros(self.n + 1, dtype=np.uint32)
        v[1:] = np.cumsum(self.A)
        return v


class PackCase(CellCase):
    kind = "pack"

    def __init__(self, name, planes, n, haploid=False, min_gq=None):
        CellCase.__init__(self, name, planes, n, 2, -1, 50, haploid, min_gq)   # the background: biallelic records, indexes -1: no class

    def cell(self, plane, record, g1, g2, cls, gq=None):
        """cls: the class 0, 1, 2 the cell packs to, or None"""
        self.put(plane, record, g1, -7 if self.haploid else g2, gq, cls)        # (haploid: gt2 is not read)

    def expected(self):
        out = np.zeros((self.planes, 3, (self.n + 63) // 64), dtype=np.uint64)
        for (plane, record), cls in self.directed.items():
            if cls is not None:
                out[plane, cls, record >> 6] |= np.uint64(1 << (record & 63))
        return out


def pack_cases():
    out = []
    c = PackCase("pack-lanes", 2, 256)
    for plane in range(2):
        k = plane                                            # (the second plane: the same lanes, other classes)
        c.cell(plane, 0, (k + 0) % 2, 0, (k + 0) % 2)                             # word 0: lane 0 alone
        c.cell(plane, 127, 1, 1 - k, 2 - k)                                       # word 1: lane 63 alone
        for lane, (g1, g2) in enumerate(((0, 0), (0, 1), (1, 1))):                # word 2: the three lanes that store
            g1, g2 = ((g1, g2), (1 - g1, 1 - g2))[k]
            c.cell(plane, 128 + lane, g1, g2, g1 + g2)
        c.cell(plane, 195, 1, k, 1 + k)                                           # word 3: lane 3 alone
    c.seams += ["lane-0-only", "lane-63-only", "lanes-0-2", "lane-3-only"]
    out.append(c)
    for n, seam in ((65, "n-64k+1"), (129, "n-64k+1"), (257, "n-256k+1"), (513, "n-256k+1")):
        c = PackCase("pack-n-%d" % n, 3, n)
        for plane in range(3):
            first, last = plane, (plane + 1) % 3
            c.cell(plane, 0, first // 2 + first % 2, first // 2, first)
            c.cell(plane, n - 1, last // 2, last // 2 + last % 2, last)
        c.seams += [seam] + ["class-%d-first" % d for d in range(3)] + ["class-%d-last" % d for d in range(3)]
        out.append(c)
    c = PackCase("pack-strays", 2, 70)
    v = 0
    for k, stray in enumerate((INT_MIN, INT_MAX, 2)):
        for g1, g2 in ((stray, 0), (0, stray), (stray, 1), (1, stray)):
            c.cell(0, v, g1, g2, None)
            c.cell(1, v, 1, 0, 1)                             # (the record is biallelic: the other plane's cell has its class)
            v += 1
        c.seams.append("index-%s" % ("int-min", "int-max", "2")[k])
    for alleles in (0, 1, 3):
        c.A[v] = c.A[v + 1] = alleles
        c.cell(0, v, 0, 0, None)
        c.cell(1, v + 1, 1 if alleles == 3 else 0, 1 if alleles == 3 else 0, None)
        v += 2
        c.seams.append("alleles-%d" % alleles)
    c.cell(0, 69, 0, 1, 1)
    out.append(c)
    for name, min_gq, cells in (("pack-gq-30", 30, ((29, None), (30, 0))), ("pack-gq-int-min", INT_MIN, ((INT_MIN, 0), (INT_MIN + 1, 0))),
                                ("pack-gq-int-max", INT_MAX, ((INT_MAX - 1, None), (INT_MAX, 0)))):
        c = PackCase(name, 2, 130, min_gq=min_gq)
        for k, (gq, cls) in enumerate(cells):
            for plane, record in ((0, k), (1, 128 + k), (0, 63 - k)):
                g = (record + plane) % 2
                c.cell(plane, record, g, g, None if cls is None else 2 * g, gq=gq)
        c.seams += ["gq-at-min-gq", "min-gq-%s" % name[8:]] + ["gq-below-min-gq"] * (min_gq != INT_MIN)
        out.append(c)
    c = PackCase("pack-haploid", 2, 130, haploid=True)
    for plane in range(2):
        for k, (g1, cls) in enumerate(((0, 0), (1, 2), (2, None), (INT_MIN, None), (INT_MAX, None), (1, 2), (0, 0))):
            c.cell(plane, (0, 1, 2, 3, 63, 64, 129)[k] if plane == 0 else (129, 128, 3, 2, 64, 63, 0)[k], g1, None, cls)
    c.seams += ["haploid-0-is-class-0", "haploid-1-is-class-2"]
    out.append(c)
    return out


REQUIRED_PACK = ["lane-0-only", "lane-63-only", "lanes-0-2", "lane-3-only", "n-64k+1", "n-256k+1", "index-int-min", "index-int-max", "index-2", "alleles-0", "alleles-1",
                 "alleles-3", "gq-at-min-gq", "gq-below-min-gq", "min-gq-30", "min-gq-int-min", "min-gq-int-max", "haploid-0-is-class-0", "haploid-1-is-class-2"] + \
                ["class-%d-%s" % (d, w) for d in range(3) for w in ("first", "last")]


def pack_holds(c, seam):
    """from the arrays and the expected planes"""
    want = c.expected()
    classed = np.zeros((c.planes, c.n), dtype=bool)           # which cells have any class, from the expected words
    cls_of = np.full((c.planes, c.n), -1)
    for d in range(3):
        bits = np.unpackbits(want[:, d].copy().view(np.uint8), axis=-1, bitorder="little")[:, :c.n].astype(bool)
        classed |= bits
        cls_of[bits] = d
    lanes = lambda plane, word: [v & 63 for v in range(64 * word, min(c.n, 64 * word + 64)) if classed[plane, v]]
    words = (c.n + 63) // 64
    if seam.startswith("lane"):
        wanted = {"lane-0-only": [0], "lane-63-only": [63], "lanes-0-2": [0, 1, 2], "lane-3-only": [3]}[seam]
        return any(lanes(p, w) == wanted for p in range(c.planes) for w in range(words))
    if seam == "n-64k+1":
        return c.n % 64 == 1 and c.n > 64 and classed[:, c.n - 1].any()
    if seam == "n-256k+1":
        return c.n % 256 == 1 and c.n > 256 and classed[:, c.n - 1].any()
    if seam.startswith("class-"):
        _, d, where = seam.split("-")
        return bool((cls_of[:, 0 if where == "first" else c.n - 1] == int(d)).any())
    two = np.broadcast_to(c.A == 2, classed.shape)
    if seam.startswith("index-"):
        x = {"int-min": INT_MIN, "int-max": INT_MAX, "2": 2}[seam[6:]]
        ok = lambda g, other: bool((two & ~classed & (g == x) & ((other == 0) | (other == 1))).any())
        return ok(c.g1, c.g2) and ok(c.g2, c.g1)
    if seam.startswith("alleles-"):
        return bool(((c.A == int(seam[8:]))[None, :] & ~classed & (c.g1 == c.g2) & ((c.g1 == 0) | (c.g1 == 1))).any())
    in01 = ((c.g1 == 0) | (c.g1 == 1)) & (c.haploid | (c.g2 == 0) | (c.g2 == 1)) & two
    if seam == "gq-at-min-gq":
        return c.min_gq is not None and bool((in01 & classed & (c.gq == c.min_gq)).any())
    if seam == "gq-below-min-gq":
        return c.min_gq is not None and bool((in01 & ~classed & (c.gq.astype(np.int64) == c.min_gq - 1)).any())
    if seam.startswith("min-gq-"):
        return c.min_gq == {"30": 30, "int-min": INT_MIN, "int-max": INT_MAX}[seam[7:]]
    if seam == "haploid-0-is-class-0":
        return c.haploid and bool((two & (c.g1 == 0) & (cls_of == 0)).any()) and not (two & (c.g1 == 0) & (cls_of != 0)).any()
    if seam == "haploid-1-is-class-2":
        return c.haploid and bool((two & (c.g1 == 1) & (cls_of == 2)).any()) and not (two & (c.g1 == 1) & (cls_of != 2)).any()
    raise KeyError(seam)


# ==== the sample table ================================================================================================================

SAMPLE_MIN_GQ = 5
CLASS_NAMES = ("TS", "TV", "INS", "DEL", "OTHER")                                 # allele classes 1..5
STATUS_NAMES = ("NORMAL", "OVERCOV", "SINGLE", "NOCOV")
BACKGROUND = dict(RECORDS=1, CALLED=1, HOM_REF=1, GQ_SUM=50, NORMAL=1, GQ_50=1)   # a called 0/0 cell of GQ 50 and status 0
GQ_EDGES = ((9, "GQ_0"), (10, "GQ_10"), (19, "GQ_10"), (20, "GQ_20"), (29, "GQ_20"), (30, "GQ_30"), (39, "GQ_30"), (40, "GQ_40"), (49, "GQ_40"), (50, "GQ_50"),
            (59, "GQ_50"), (60, "GQ_60"), (69, "GQ_60"), (70, "GQ_70"), (79, "GQ_70"), (80, "GQ_80"), (89, "GQ_80"), (90, "GQ_90"), (99, "GQ_90"), (100, "GQ_90"))


def _kinds():
    """name -> (gt1, gt2, gq, status, the slots the cell adds to), in records of six alleles REF, TS, TV, INS, DEL, OTHER under
    min_gq = 5"""
    called = dict(RECORDS=1, CALLED=1, GQ_SUM=50, NORMAL=1, GQ_50=1)
    k = {
        "masked": (0, 0, 4, 0, dict(RECORDS=1, MASKED=1, NORMAL=1, GQ_0=1)),
        "masked-stray": (-1, 9, 4, 0, dict(RECORDS=1, MASKED=1, NORMAL=1, GQ_0=1)),       # masked is decided first: not BAD, and in the histogram
        "bad": (6, 0, 50, 0, dict(RECORDS=1, BAD=1, NORMAL=1)),                           # index A; a bad cell is not in the histogram
        "bad-negative": (0, -1, 50, 0, dict(RECORDS=1, BAD=1, NORMAL=1)),
        "hom-alt": (1, 1, 50, 0, dict(called, HOM_ALT=1, TS=1)),
        "het": (0, 2, 50, 0, dict(called, HET=1, TV=1)),
        "het-alt": (3, 4, 50, 0, dict(called, HET=1, HET_ALT=1, INS=1, DEL=1)),
        "gq-at-min-gq": (0, 0, 5, 0, dict(RECORDS=1, CALLED=1, HOM_REF=1, GQ_SUM=5, NORMAL=1, GQ_0=1)),
    }
    for c, name in enumerate(CLASS_NAMES, start=1):
        k["class-%d-gt1" % c] = (c, 0, 50, 0, dict(called, HET=1, **{name: 1}))
        k["class-%d-gt2" % c] = (0, c, 50, 0, dict(called, HET=1, **{name: 1}))
    for s in (0, 1, 2, 3, 7):
        adds = dict(RECORDS=1, CALLED=1, HOM_REF=1, GQ_SUM=50, GQ_50=1)
        if s < 4:
            adds[STATUS_NAMES[s]] = 1                                                     # (any other code: nothing)
        k["status-%d" % s] = (0, 0, 50, s, adds)
    for q, bin_name in GQ_EDGES:
        k["gq-%d" % q] = (0, 0, q, 0, dict({"RECORDS": 1, "CALLED": 1, "HOM_REF": 1, "GQ_SUM": q, "NORMAL": 1}, **{bin_name: 1}))
    return k


KINDS = _kinds()
KIND_NAMES = tuple(KINDS)
SAMPLE_SPOTS = ("0", "63", "64", "255", "256", "run-1", "run", "run+64", "last")


def sample_spot(name, n, run):
    return {"0": 0, "63": 63, "64": 64, "255": 255, "256": 256, "run-1": run - 1, "run": run, "run+64": run + 64, "last": n - 1}[name]


class SampleCase(CellCase):
    kind = "sample"

    def __init__(self, name, planes, n, alleles=6, gq=50, min_gq=SAMPLE_MIN_GQ, status=True, classes=True, cut=None):
        CellCase.__init__(self, name, planes, n, alleles, 0, gq, False, min_gq)
        self.status = np.zeros((planes, n), dtype=np.uint8) if status else None
        self.classes = classes                                # every record's alleles are REF, TS, TV, INS, DEL, OTHER, TS, ..
        self.cov = None                                       # [planes, slots], made by the case that wants it
        self.adds = [dict() for _ in range(planes)]           # per plane what the directed cells and the case's own rows add
        self.background = None                                # what a cell the case did not touch adds (None: stated by the case in adds)
        self.start = None
        self.cut = n // 2 if cut is None else cut
        assert 0 < self.cut < n

    def add(self, plane, **slots):
        for k, v in slots.items():
            self.adds[plane][k] = self.adds[plane].get(k, 0) + v

    def kind_cell(self, plane, record, kind):
        g1, g2, gq, st, adds = KINDS[kind]
        self.put(plane, record, g1, g2, gq, kind)
        self.status[plane, record] = st
        self.add(plane, **adds)

    def allele_class(self):
        if not self.classes:
            return None
        slots = int(self.A.sum())
        within = np.arange(slots) - np.repeat(np.cumsum(self.A) - self.A, self.A)
        return np.where(within == 0, 0, (within - 1) % 5 + 1).astype(np.uint8)

    def expected(self):
        """-> uint64 [planes, 32], two's complement where a sum is negative"""
        out = np.zeros((self.planes, SLOTS), dtype=np.uint64)
        for p in range(self.planes):
            total = dict(self.adds[p])
            if self.background is not None:
                rest = self.n - sum(1 for (plane, _) in self.directed if plane == p)
                for k, v in self.background.items():
                    total[k] = total.get(k, 0) + rest * v
            for k, v in total.items():
                out[p, SS[k]] = np.uint64(v % (1 << 64))
        return out

    def start_table(self):
        return np.zeros((self.planes, SLOTS), dtype=np.uint64) if self.start is None else self.start.copy()


# 3 planes: 682 runs at most, so 682 steps of 256 and a record are runs of 512 records, the last of one record
N_VARS_3 = (2048 // 3) * 256 + 1
SAMPLE_SHAPES = ((64, 8193), (64, 20011), (1, 524289), (3, N_VARS_3))


_BUILT = (None, None)                                       # the arrays of the kind case last asked for: one at a time


class KindCase(SampleCase):
    """background cells and kinds of cell at the spots of the plan's runs; the arrays are made when asked for and those of one case
    are kept at a time (a case per kind on 524,289 records would hold 300 MB otherwise)"""

    def __init__(self, name, planes, n, cut):
        self.name, self.planes, self.n, self.haploid, self.min_gq, self.cut = name, planes, n, False, SAMPLE_MIN_GQ, cut
        self.seams, self.directed, self.adds = [], {}, [dict() for _ in range(planes)]
        self.classes, self.cov, self.start, self.background = True, None, None, BACKGROUND
        assert 0 < cut < n

    def kind_cell(self, plane, record, kind):
        assert (plane, record) not in self.directed and 0 <= plane < self.planes and 0 <= record < self.n
        self.directed[(plane, record)] = kind
        self.add(plane, **KINDS[kind][4])

    def _built(self):
        global _BUILT
        if _BUILT[0] is not self:
            P, n = self.planes, self.n
            x = dict(g1=np.zeros((P, n), dtype=np.int32), g2=np.zeros((P, n), dtype=np.int32), gq=np.full((P, n), 50, dtype=np.int32),
                     status=np.zeros((P, n), dtype=np.uint8), A=np.full(n, 6, dtype=np.int64))
            for (plane, record), kind in self.directed.items():
                x["g1"][plane, record], x["g2"][plane, record], x["gq"][plane, record], x["status"][plane, record] = KINDS[kind][:4]
            _BUILT = (self, x)
        return _BUILT[1]

    g1 = property(lambda self: self._built()["g1"])
    g2 = property(lambda self: self._built()["g2"])
    gq = property(lambda self: self._built()["gq"])
    status = property(lambda self: self._built()["status"])
    A = property(lambda self: self._built()["A"])


def _sample_kind_cases(planes, n):
    """every kind of cell at every spot of the plan's runs, in every shape.  A plane has nine spots: with 64 planes one case holds the
    whole cross, with fewer a case holds one kind per plane at all nine"""
    run, n_runs = sample_plan(n, planes)
    spots = [sample_spot(s, n, run) for s in SAMPLE_SPOTS]
    assert len(set(spots)) == len(spots) and max(spots) == n - 1 and n_runs > 1
    K = len(KIND_NAMES)
    shape = "%dx%d" % (planes, n)
    out = []
    if planes >= K:
        c = KindCase("sample-kinds-" + shape, planes, n, cut=run)
        for ki, kind in enumerate(KIND_NAMES):
            for si, record in enumerate(spots):
                c.kind_cell((ki + 7 * si) % planes, record, kind)
        c.seams += ["kind-%s@%s#%s" % (kind, s, shape) for kind in KIND_NAMES for s in SAMPLE_SPOTS]
        out.append(c)
    else:
        for first in range(0, K, planes):
            kinds = [KIND_NAMES[(first + p) % K] for p in range(planes)]
            c = KindCase("sample-kinds-%s-%s" % (shape, kinds[0]), planes, n, cut=run)
            for p, kind in enumerate(kinds):
                for record in spots:
                    c.kind_cell(p, record, kind)
            c.seams += ["kind-%s@%s#%s" % (kind, s, shape) for kind in dict.fromkeys(kinds) for s in SAMPLE_SPOTS]
            out.append(c)
    for c in out:
        c.seams.append("shape-" + shape)
    return out


def sample_cases():
    out = [c for planes, n in SAMPLE_SHAPES for c in _sample_kind_cases(planes, n)]
    n = 600                                                   # three workgroups of 256 records to a plane
    c = SampleCase("sample-gq-extremes", 5, n, alleles=1, gq=0, min_gq=None, status=False, classes=False, cut=256)
    c.gq[0], c.gq[1], c.gq[4] = INT_MIN, INT_MAX, 50
    c.add(0, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=n * INT_MIN, GQ_0=n)          # a negative sum; a negative GQ is in bin 0
    c.add(1, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=n * INT_MAX, GQ_90=n)
    c.gq[2, 10], c.gq[2, 20] = INT_MAX, -INT_MAX                                  # cancel inside one workgroup
    c.add(2, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=0, GQ_0=n - 1, GQ_90=1)
    c.gq[3, 10], c.gq[3, 300] = 7777, -7777                                       # cancel across two
    c.add(3, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=0, GQ_0=n - 1, GQ_90=1)
    c.add(4, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=50 * n, GQ_50=n)
    c.seams += ["gq-plane-int-min", "gq-plane-int-max", "gq-sum-zero-one-workgroup", "gq-sum-zero-two-workgroups"]
    out.append(c)
    n = 300
    c = SampleCase("sample-min-gq-int-min", 2, n, alleles=1, gq=INT_MIN, min_gq=INT_MIN, status=False, classes=False)
    c.gq[1] = -1
    c.add(0, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=n * INT_MIN, GQ_0=n)          # nothing is below INT32_MIN: nothing is masked
    c.add(1, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=-n, GQ_0=n)
    c.seams.append("min-gq-int-min")
    out.append(c)
    c = SampleCase("sample-min-gq-int-max", 2, n, alleles=1, gq=INT_MAX - 1, min_gq=INT_MAX, status=False, classes=False)
    c.gq[1] = INT_MAX
    c.add(0, RECORDS=n, MASKED=n, GQ_90=n)                                        # (a masked cell is in the histogram, not in the sum)
    c.add(1, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=n * INT_MAX, GQ_90=n)
    c.seams.append("min-gq-int-max")
    out.append(c)
    # indexes INT32_MIN, INT32_MAX and A in records of 0, 1, 2 and 70 alleles, twice over: 8 records
    c = SampleCase("sample-indexes", 5, 8, min_gq=None, status=False, cut=4)
    c.A[:] = (0, 1, 2, 70) * 2
    c.g1[0], c.g2[1] = INT_MIN, INT_MAX
    c.g1[2] = c.A
    c.g1[4] = c.g2[4] = c.A - 1
    for p in range(3):
        c.add(p, RECORDS=8, BAD=8)
    c.add(3, RECORDS=8, BAD=2, CALLED=6, HOM_REF=6, GQ_SUM=300, GQ_50=6)          # 0/0: bad where the record has no allele at all
    c.add(4, RECORDS=8, BAD=2, CALLED=6, HOM_REF=2, HOM_ALT=4, TS=2, DEL=2, GQ_SUM=300, GQ_50=6)   # A - 1: -1, 0, 1 (TS), 69 (the 69th ALT: class (68 mod 5) + 1 = DEL)
    c.cov = np.ones((5, int(c.A.sum())), dtype=np.uint32)
    for p in range(5):
        c.add(p, COV_SUM=146)
    c.seams += ["index-%s-in-A%d" % (x, A) for x in ("int-min", "int-max", "A") for A in (0, 1, 2, 70)] + ["records-without-slots-among-others"]
    out.append(c)
    # a 70-allele record on either side of the first run seam of 64 planes x 8,193 records (run 512), every coverage 2^32 - 1
    n = 8193
    c = SampleCase("sample-cov-max", 64, n, alleles=2, min_gq=None, status=False, classes=False, cut=512)
    c.A[511] = c.A[512] = 70
    c.cov = np.repeat(np.arange(1, 65, dtype=np.uint32)[:, None], int(c.A.sum()), axis=1)
    c.cov[:, 2 * 511:2 * 511 + 140] = U32_MAX
    for p in range(64):
        c.add(p, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=50 * n, GQ_50=n, COV_SUM=(p + 1) * 2 * (n - 2) + 140 * U32_MAX)
    c.seams.append("cov-max-70-alleles-at-run-seam")
    out.append(c)
    n = 300
    c = SampleCase("sample-accumulate-wrap", 2, n, alleles=2, min_gq=None, status=False, classes=False)
    c.cov = np.full((2, 2 * n), 3, dtype=np.uint32)
    for p in range(2):
        c.add(p, RECORDS=n, CALLED=n, HOM_REF=n, GQ_SUM=50 * n, GQ_50=n, COV_SUM=6 * n)
    c.start = np.full((2, SLOTS), 7, dtype=np.uint64)
    c.start[:, SS["GQ_SUM"]] = np.uint64(M64)                                     # -1
    c.start[:, SS["COV_SUM"]] = np.uint64(M64)                                    # the sum wraps, by definition
    c.seams += ["accumulate-onto-gq-sum-minus-1", "accumulate-cov-sum-wraps"]
    out.append(c)
    c = SampleCase("sample-no-slots", 3, n, alleles=0, min_gq=None, classes=False)
    for p in range(3):
        c.add(p, RECORDS=n, BAD=n, NORMAL=n)                                      # index 0 of a record without alleles is outside it
    c.seams.append("records-without-slots")
    out.append(c)
    return out


REQUIRED_SAMPLE = ["kind-%s@%s#%dx%d" % ((k, s) + shape) for shape in SAMPLE_SHAPES for k in KIND_NAMES for s in SAMPLE_SPOTS] + ["shape-%dx%d" % s for s in SAMPLE_SHAPES] + \
    ["gq-plane-int-min", "gq-plane-int-max", "gq-sum-zero-one-workgroup", "gq-sum-zero-two-workgroups", "min-gq-int-min", "min-gq-int-max",
     "records-without-slots-among-others", "cov-max-70-alleles-at-run-seam", "accumulate-onto-gq-sum-minus-1", "accumulate-cov-sum-wraps", "records-without-slots"] + \
    ["index-%s-in-A%d" % (x, A) for x in ("int-min", "int-max", "A") for A in (0, 1, 2, 70)]


def sample_holds(c, seam):
    """from the arrays, the plan of the shape and the expected table"""
    run, n_runs = sample_plan(c.n, c.planes)
    want = c.expected().astype(np.int64)                      # (two's complement: a negative sum reads negative)
    q = c.gq.astype(np.int64)
    if seam.startswith("kind-"):
        seam, _, shape = seam.partition("#")
        if shape != "%dx%d" % (c.planes, c.n):
            return False
        kind, _, spot = seam[5:].rpartition("@")
        g1, g2, gq, st, _ = KINDS[kind]
        v = sample_spot(spot, c.n, run)
        if spot.startswith("run") and n_runs < 2:
            return False
        at = (c.g1[:, v] == g1) & (c.g2[:, v] == g2) & (c.gq[:, v] == gq) & (c.status[:, v] == st) & (c.A[v] == 6) & (c.min_gq == SAMPLE_MIN_GQ)
        return bool(at.any())
    if seam.startswith("shape-"):
        return seam == "shape-%dx%d" % (c.planes, c.n) and n_runs > 1 and run > 256      # (a wave takes several steps, a plane several runs)
    if seam == "gq-plane-int-min":
        return bool(((q == INT_MIN).all(axis=1) & (want[:, SS["GQ_SUM"]] < 0) & (want[:, SS["GQ_0"]] == c.n)).any())
    if seam == "gq-plane-int-max":
        return bool(((q == INT_MAX).all(axis=1) & (want[:, SS["GQ_SUM"]] == c.n * INT_MAX)).any())
    if seam in ("gq-sum-zero-one-workgroup", "gq-sum-zero-two-workgroups"):
        for p in range(c.planes):
            nz = np.flatnonzero(q[p])
            if nz.size == 2 and q[p].sum() == 0 and want[p, SS["GQ_SUM"]] == 0 and c.min_gq is None:
                if (nz[0] // run == nz[1] // run) == (seam == "gq-sum-zero-one-workgroup"):
                    return True
        return False
    if seam == "min-gq-int-min":
        return c.min_gq == INT_MIN and bool((q == INT_MIN).any()) and not want[:, SS["MASKED"]].any()
    if seam == "min-gq-int-max":
        return c.min_gq == INT_MAX and bool((q == INT_MAX - 1).any() and (q == INT_MAX).any()) and set(want[:, SS["MASKED"]]) == {0, c.n}
    if seam.startswith("index-"):
        name, _, A = seam[6:].partition("-in-A")
        g = {"int-min": INT_MIN, "int-max": INT_MAX, "A": int(A)}[name]
        return bool(((c.A == int(A))[None, :] & ((c.g1 == g) | (c.g2 == g))).any())
    if seam == "records-without-slots-among-others":
        return bool((c.A == 0).any() and (c.A > 0).any())
    if seam == "records-without-slots":
        return bool((c.A == 0).all()) and c.n > 256
    if seam == "cov-max-70-alleles-at-run-seam":
        vao = c.vao().astype(np.int64)
        ok = n_runs > 1 and c.cov is not None
        for v in (run - 1, run):
            ok = ok and c.A[v] == 70 and bool((c.cov[:, vao[v]:vao[v + 1]] == U32_MAX).all())
        return bool(ok)
    if seam == "accumulate-onto-gq-sum-minus-1":
        return c.start is not None and bool((c.start[:, SS["GQ_SUM"]] == np.uint64(M64)).all()) and bool((want[:, SS["GQ_SUM"]] > 0).all())
    if seam == "accumulate-cov-sum-wraps":
        return c.start is not None and bool((c.start[:, SS["COV_SUM"]] == np.uint64(M64)).all()) and bool((want[:, SS["COV_SUM"]] > 0).all())
    raise KeyError(seam)


# ==== site tags and site genotype counts ===============================================================================================

SITE_MIN_GQ = 30
SITE_ALLELES = (0, 1, 2, 8, 9, 127, 128, 129, 255, 256, 257)


class Geno:
    """a cell and what both kernels make of it: `tags` the alleles mg_site_counts counts (and `called`: whether NS counts the cell),
    `geno` ("hom", a), ("het", a, b) or None for mg_site_geno_counts"""

    def __init__(self, g1, g2, tags, geno, called=True):
        self.g1, self.g2, self.tags, self.geno, self.called = g1, g2, tuple(tags), geno, called

    def masked(self):
        return Geno(self.g1, self.g2, (), None, called=False)


def hom(a):
    return Geno(a, a, (a, a), ("hom", a))


def het(a, b):
    assert a != b
    return Geno(a, b, (a, b), ("het", a, b))


def stray1(valid, stray, first=True):
    """one index inside the record, one outside: the tags count the one inside, the genotype counts nothing"""
    return Geno(valid, stray, (valid,), None) if first else Geno(stray, valid, (valid,), None)


def stray2(s1, s2):
    return Geno(s1, s2, (), None)


def genotypes(A):
    """the cells a record of A alleles is given, each written down with A in hand"""
    g = []
    if A >= 1:
        g += [hom(0), hom(A - 1), stray1(0, A), stray1(A - 1, INT_MIN, first=False), stray1(0, INT_MAX), stray1(A - 1, A, first=False)]
    if A >= 2:
        g += [het(0, A - 1), het(A - 1, 0), het(1, 0)]
    g += [stray2(A, A), stray2(INT_MIN, INT_MAX), stray2(INT_MAX, INT_MIN)]
    for x in (127, 128, 255, 256):
        if x < A:
            g += [hom(x), het(0, x), het(x, 0)]
        else:
            g += [stray2(x, x)] + ([stray1(0, x)] if A >= 1 else [])
    if A >= 129:
        g += [het(5, 128), het(128, 5), het(127, 128), hom(128)]                  # rounds 1 and 2 of SITE_BINS
    if A >= 257:
        g += [het(3, 256), het(256, 3), het(255, 256), het(130, 256), hom(200)]   # and round 3
    return g


# a record type: ("mixed", A) the cells of genotypes(A) dealt over the planes; ("all-hom", A, a) / ("all-het", A, a, b) every plane the same
SITE_TYPES = tuple(("mixed", A) for A in SITE_ALLELES) + (("all-hom", 8, 7), ("all-hom", 9, 8), ("all-hom", 129, 128), ("all-het", 128, 0, 127), ("all-het", 257, 1, 256))
SITE_PATTERNS = ("all", "only-first", "only-last")


class SiteCase:
    kind = "site"

    def __init__(self, name, planes, n, rot, groups):
        self.name, self.planes, self.n, self.groups = name, planes, n, groups     # groups: the plane cuts of the accumulating calls
        self.min_gq = SITE_MIN_GQ
        self.seams = []
        self.cells = [[None] * n for _ in range(planes)]
        self.A = np.zeros(n, dtype=np.int64)
        for v in range(n):
            t = SITE_TYPES[(v + rot) % len(SITE_TYPES)]
            self.A[v] = A = t[1]
            if t[0] == "mixed":
                g = genotypes(A)
                pattern = SITE_PATTERNS[(v + 2 * rot) % 3]
                for p in range(planes):
                    cell = g[(p + rot) % len(g)]
                    keep = pattern == "all" or (pattern == "only-first" and p == 0) or (pattern == "only-last" and p == planes - 1)
                    self.cells[p][v] = cell if keep else cell.masked()
            else:
                for p in range(planes):
                    self.cells[p][v] = hom(t[2]) if t[0] == "all-hom" else het(t[2], t[3])
        self._arrays()

    def _arrays(self):
        P, n = self.planes, self.n
        self.g1 = np.array([[c.g1 for c in row] for row in self.cells], dtype=np.int32).reshape(P, n)
        self.g2 = np.array([[c.g2 for c in row] for row in self.cells], dtype=np.int32).reshape(P, n)
        # a called cell stands exactly at min_gq, a masked one just below
        self.gq = np.array([[SITE_MIN_GQ if c.called else SITE_MIN_GQ - 1 for c in row] for row in self.cells], dtype=np.int32).reshape(P, n)

    def vao(self):
        v = np.zeros(self.n + 1, dtype=np.uint32)
        v[1:] = np.cumsum(self.A)
        return v

    def expected(self, lo=0, hi=None):
        """-> (ac, ns), (n, het, hom) of the planes [lo, hi), uint32"""
        vao = self.vao().astype(np.int64)
        slots = int(vao[-1])
        ac, ns = np.zeros(slots, dtype=np.uint32), np.zeros(self.n, dtype=np.uint32)
        n_us, n_het, n_hom = np.zeros(self.n, dtype=np.uint32), np.zeros(slots, dtype=np.uint32), np.zeros(slots, dtype=np.uint32)
        for row in self.cells[lo:hi]:
            for v, c in enumerate(row):
                ns[v] += c.called
                for a in c.tags:
                    ac[vao[v] + a] += 1
                if c.geno is not None:
                    n_us[v] += 1
                    if c.geno[0] == "hom":
                        n_hom[vao[v] + c.geno[1]] += 1
                    else:
                        n_het[vao[v] + c.geno[1]] += 1
                        n_het[vao[v] + c.geno[2]] += 1
        return (ac, ns), (n_us, n_het, n_hom)


class NoSlotsSiteCase(SiteCase):
    """records without alleles: both kernels have nothing to count into but NS"""

    def __init__(self):
        self.name, self.planes, self.n, self.groups, self.min_gq, self.seams = "site-no-slots", 3, 5, (0, 1, 3), SITE_MIN_GQ, ["records-without-slots"]
        self.A = np.zeros(5, dtype=np.int64)
        self.cells = [[stray2(0, 0) if (p + v) % 3 else stray2(0, 0).masked() for v in range(5)] for p in range(3)]
        self._arrays()


def site_cases():
    out = []
    for pi, planes in enumerate((1, 2, 63, 64)):
        for rot in range(len(SITE_TYPES)):
            n = len(SITE_TYPES) + (rot + pi) % 4
            cut = (0, planes) if planes == 1 else (0, 1, planes) if rot % 2 else (0, planes // 2, planes)
            out.append(SiteCase("site-%dp-rot%d" % (planes, rot), planes, n, rot, cut))
    for planes, groups in ((128, (0, 64, 128)), (130, (0, 64, 128, 130))):
        for rot in (0, 5, 10, 13):
            out.append(SiteCase("site-%dp-rot%d" % (planes, rot), planes, len(SITE_TYPES) + 1, rot, groups))
    out.append(NoSlotsSiteCase())
    for c in out[:-1]:
        c.seams = [s for s in REQUIRED_SITE if s != "records-without-slots" and site_holds(c, s)]   # a case claims what its rotation gives it;
    return out                                                                    # the CPU test checks the claims again and that none is missing


REQUIRED_SITE = ["A-%d@record-%s" % (A, r) for A in SITE_ALLELES for r in ("0", "3", "4", "last")] + ["n-mod-4-is-%d" % k for k in range(4)] + \
    ["planes-%d" % p for p in (1, 2, 63, 64)] + ["only-plane-0", "only-plane-63", "only-last-plane-of-63", "all-planes-called"] + \
    ["index-%s" % x for x in ("0", "A-1", "A", "127-inside", "127-outside", "128-inside", "128-outside", "255-inside", "255-outside", "256-inside", "256-outside",
                              "int-min", "int-max")] + \
    ["het-round1-round2", "het-round2-round1", "het-round1-round3", "het-round3-round1", "het-round2-round3", "hom-round2", "all-64-hom-one-lds-bin", "all-64-hom-ballots",
     "all-64-het-same-two", "one-stray-index", "gq-at-min-gq", "gq-below-min-gq", "groups-2-of-64", "groups-3-of-64-64-2", "records-without-slots"]


def site_holds(c, seam):
    """from the arrays alone"""
    A = c.A[None, :]
    g1, g2 = c.g1.astype(np.int64), c.g2.astype(np.int64)
    called = c.gq >= c.min_gq
    in1, in2 = (g1 >= 0) & (g1 < A), (g2 >= 0) & (g2 < A)
    if seam.startswith("A-"):
        a, _, r = seam[2:].partition("@record-")
        return c.n > 5 and c.planes <= 64 and c.A[c.n - 1 if r == "last" else int(r)] == int(a)
    if seam.startswith("n-mod-4-is-"):
        return c.n % 4 == int(seam[-1]) and c.planes <= 64
    if seam.startswith("planes-"):
        return c.planes == int(seam[7:])
    if seam in ("only-plane-0", "only-plane-63", "only-last-plane-of-63"):
        need, p = {"only-plane-0": (None, 0), "only-plane-63": (64, 63), "only-last-plane-of-63": (63, 62)}[seam]
        if c.planes < 2 or (need is not None and c.planes != need):
            return False
        return bool((called[p] & (called.sum(axis=0) == 1)).any())
    if seam == "all-planes-called":
        return c.planes >= 2 and bool(called.all(axis=0).any())
    if seam.startswith("index-"):
        x = seam[6:]
        both = lambda m1, m2: bool((called & m1).any() and (called & m2).any())
        if x == "0":
            return both(g1 == 0, g2 == 0)
        if x == "A-1":
            return both((g1 == A - 1) & (A >= 2), (g2 == A - 1) & (A >= 2))
        if x == "A":
            return both(g1 == A, g2 == A)
        if x in ("int-min", "int-max"):
            v = INT_MIN if x == "int-min" else INT_MAX
            return both(g1 == v, g2 == v)
        v, where = x.split("-")
        v = int(v)
        ok = (A > v) if where == "inside" else (A <= v)
        return both((g1 == v) & ok, (g2 == v) & ok)
    rnd = lambda g: g // SITE_BINS
    usable = called & in1 & in2 & (A > SITE_BALLOT_MAX)
    if seam.startswith("het-round"):
        r1, r2 = int(seam[9]) - 1, int(seam[-1]) - 1
        return bool((usable & (g1 != g2) & (rnd(g1) == r1) & (rnd(g2) == r2)).any())
    if seam == "hom-round2":
        return bool((usable & (g1 == g2) & (rnd(g1) == 1)).any())
    if seam.startswith("all-64-"):
        if c.planes != 64:
            return False
        same = called.all(axis=0) & (g1 == g1[0]).all(axis=0) & (g2 == g2[0]).all(axis=0) & in1[0] & in2[0]
        if seam == "all-64-hom-one-lds-bin":
            return bool((same & (g1[0] == g2[0]) & (c.A > SITE_BALLOT_MAX)).any())
        if seam == "all-64-hom-ballots":
            return bool((same & (g1[0] == g2[0]) & (c.A <= SITE_BALLOT_MAX)).any())
        return bool((same & (g1[0] != g2[0]) & (c.A > SITE_BALLOT_MAX) & (rnd(g1[0]) != rnd(g2[0]))).any())
    if seam == "one-stray-index":
        return bool((called & (in1 != in2)).any())
    if seam == "gq-at-min-gq":
        return bool((c.gq == c.min_gq).any())
    if seam == "gq-below-min-gq":
        return bool((c.gq == c.min_gq - 1).any())
    if seam == "groups-2-of-64":
        return tuple(c.groups) == (0, 64, 128)
    if seam == "groups-3-of-64-64-2":
        return tuple(c.groups) == (0, 64, 128, 130)
    if seam == "records-without-slots":
        return bool((c.A == 0).all())
    raise KeyError(seam)


# ==== all of them =====================================================================================================================

REQUIRED = {"pair": _required_pair(), "pack": REQUIRED_PACK, "sample": REQUIRED_SAMPLE, "site": REQUIRED_SITE}
_CASES = None


def cases():
    """every case, made once"""
    global _CASES
    if _CASES is None:
        _CASES = pair_cases() + pack_cases() + sample_cases() + site_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES
