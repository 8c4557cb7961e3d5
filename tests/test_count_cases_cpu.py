"""The case table of tests/count_cases.py, proved without a GPU: every case's written-down expectation is what the numpy restatements
of the existing test files make of its inputs (pack_plain, sample_counts_plain, counts_numpy, geno_counts_plain, and for the pair
table a word-wise popcount held against pair_plain wherever that one's einsum fits); every case holds every seam it claims, checked
from its inputs and the restated plans; every seam of the lists is claimed by at least one case; and no case is left out of
tests/test_gpu_count_edges.py."""
import numpy as np
import pytest

import count_cases as cc
from site_stats_model import geno_counts_plain
from test_gpu_site_tags import counts_numpy
from test_pairs_cpu import pack_plain, pair_plain
from test_sample_stats_cpu import SLOT_NAMES, SS, sample_counts_plain

CASES = cc.cases()
of_kind = lambda kind: pytest.mark.parametrize("case", [c for c in CASES if c.kind == kind], ids=lambda c: c.name)


def pair_words_plain(a, b=None):
    """-> uint64 [n_a, n_b, 3, 3]: the definition word by word, popcount(A[i][da][w] & B[j][db][w]) summed over w.  A row without a
    bit meets nothing and is passed over."""
    b = a if b is None else b
    out = np.zeros((a.shape[0], b.shape[0], 3, 3), dtype=np.uint64)
    rows_b = [(j, db) for j in range(b.shape[0]) for db in range(3) if b[j, db].any()]
    if not rows_b:
        return out
    stack = np.stack([b[j, db] for j, db in rows_b])
    for i in range(a.shape[0]):
        for da in range(3):
            if a[i, da].any():
                sums = np.bitwise_count(stack & a[i, da][None, :]).sum(axis=1, dtype=np.uint64)
                for (j, db), s in zip(rows_b, sums):
                    out[i, j, da, db] = s
    return out


def test_the_word_wise_restatement_on_cases_small_enough_to_read():
    a = np.array([[[0b1011, 0], [0, 1 << 63], [0, 0]], [[0b0110, 0], [0, 0], [cc.M64, cc.M64]]], dtype=np.uint64)
    got = pair_words_plain(a)
    assert got[0, 0, 0, 0] == 3 and got[0, 1, 0, 0] == 1 and got[0, 1, 0, 2] == 3 and got[0, 1, 1, 2] == 1 and got[1, 1, 2, 2] == 128 and got[0, 0, 0, 1] == 0
    assert np.array_equal(got, got.transpose(1, 0, 3, 2)) and np.array_equal(got, pair_plain(a)) and np.array_equal(pair_words_plain(a, a[:1]), got[:, :1])
    rng = np.random.default_rng(3)
    x, y = rng.integers(0, 1 << 64, size=(5, 3, 70), dtype=np.uint64), rng.integers(0, 1 << 64, size=(3, 3, 70), dtype=np.uint64)
    assert np.array_equal(pair_words_plain(x, y), pair_plain(x, y)) and np.array_equal(pair_words_plain(x), pair_plain(x))


def _first_pair_difference(got, want):
    i, j, da, db = (int(x[0]) for x in np.nonzero(got != want))
    return "first difference at (i, j, da, db) = (%d, %d, %d, %d): %d, expected %d" % (i, j, da, db, int(got[i, j, da, db]), int(want[i, j, da, db]))


@of_kind("pair")
def test_pair_case(case):
    a, b = case.planes()
    want = case.expected()
    assert a.nbytes <= 13_000_000 and (b is None or b.nbytes <= 13_000_000)
    got = pair_words_plain(a, b)
    assert np.array_equal(got, want), _first_pair_difference(got, want)
    if case.n_words <= 2048:
        assert np.array_equal(pair_plain(a, b), want)
    if case.symmetric:
        assert np.array_equal(want, want.transpose(1, 0, 3, 2))
    assert case.seams and len(set(case.seams)) == len(case.seams)
    for seam in case.seams:
        assert seam in cc.REQUIRED["pair"], seam
        assert cc.pair_holds(case, seam, a, b, want), "%s does not hold %s" % (case.name, seam)
    bb = a if b is None else b
    if case.decoys:
        # a placement counts exactly once in its own entry; a decoy's bit is shared by no row of the other operand (B is A: by no other
        # row), so it counts nothing between two rows; and one word off, at every placement, it would: an entry that must be 0 reads 1
        for pl in case.placements:
            i, da, j, db, word, bit = pl
            if not (case.symmetric and (i, da) == (j, db)):   # (a row of A against itself counts every bit it holds, its decoys too)
                assert int(want[i, j, da, db]) == sum(q[:4] == pl[:4] or (case.symmetric and (q[2], q[3], q[0], q[1]) == pl[:4]) for q in case.placements)
            for step in (-1, 1):
                if 0 <= word + step < case.n_words:
                    assert cc.shifted_entries(case, a, bb, want, pl, step), "%s: word %d read %+d off changes no entry" % (case.name, word, step)
        for jd, dd, word, bit in case.decoys:
            holders = [(p, d) for p in range(a.shape[0]) for d in range(3) if (int(a[p, d, word]) >> bit) & 1 and not case.is_ones("a", p, d)]
            assert holders == ([(jd, dd)] if case.symmetric else []) and (int(bb[jd, dd, word]) >> bit) & 1
    if case.start is not None:
        assert case.start.shape == want.shape and case.start.dtype == np.uint64


@of_kind("pack")
def test_pack_case(case):
    want = case.expected()
    got = pack_plain(case.g1, None if case.haploid else case.g2, case.gq, case.haploid, case.vao(), case.min_gq)
    assert np.array_equal(got, want), np.argwhere(got != want)[:3]
    assert want.any() and not (want[:, 0] & want[:, 1]).any() and not (want[:, 0] & want[:, 2]).any() and not (want[:, 1] & want[:, 2]).any()
    for seam in case.seams:
        assert seam in cc.REQUIRED["pack"], seam
        assert cc.pack_holds(case, seam), "%s does not hold %s" % (case.name, seam)


def _first_slot_difference(got, want):
    p, k = (int(x[0]) for x in np.nonzero(got != want))
    return "first difference at (plane, slot) = (%d, %s): %d, expected %d" % (p, SLOT_NAMES[k] if k < len(SLOT_NAMES) else k, int(got[p, k]), int(want[p, k]))


@of_kind("sample")
def test_sample_case(case):
    want = case.expected()
    got = sample_counts_plain(case.g1, case.g2, case.gq, False, case.vao(), case.status, case.cov, case.allele_class(), case.min_gq)
    assert np.array_equal(got, want), _first_slot_difference(got, want)
    assert (want[:, SS["RECORDS"]] == case.n).all() and np.array_equal(want[:, SS["RECORDS"]], want[:, SS["MASKED"]] + want[:, SS["BAD"]] + want[:, SS["CALLED"]])
    assert case.cov is None or case.cov.shape == (case.planes, int(case.A.sum()))
    for seam in case.seams:
        assert seam in cc.REQUIRED["sample"], seam
        assert cc.sample_holds(case, seam), "%s does not hold %s" % (case.name, seam)
    # the two halves of an accumulating run are cases of the same restatement: the cut is a record of the case
    assert 0 < case.cut < case.n


@of_kind("site")
def test_site_case(case):
    vao = case.vao()
    (ac, ns), (n_us, het, hom) = case.expected()
    want_ac, want_ns = counts_numpy(case.g1, case.g2, case.gq, False, vao, case.min_gq)
    assert np.array_equal(ac, want_ac) and np.array_equal(ns, want_ns), case.name
    want_geno = geno_counts_plain(case.g1, case.g2, case.gq, False, vao, case.min_gq)
    for g, w, what in zip((n_us, het, hom), want_geno, ("n", "het", "hom")):
        assert np.array_equal(g, w), what
    # the groups of the accumulating calls add up to the whole
    assert case.groups[0] == 0 and case.groups[-1] == case.planes and all(0 < hi - lo <= 64 for lo, hi in zip(case.groups, case.groups[1:]))
    parts = [case.expected(lo, hi) for lo, hi in zip(case.groups, case.groups[1:])]
    assert np.array_equal(sum(p[0][0] for p in parts), ac) and np.array_equal(sum(p[1][2] for p in parts), hom)
    assert case.seams and len(set(case.seams)) == len(case.seams)
    for seam in case.seams:
        assert seam in cc.REQUIRED["site"], seam
        assert cc.site_holds(case, seam), "%s does not hold %s" % (case.name, seam)


def test_what_the_site_cases_are_meant_to_have():
    """the claims of the site cases are collected from their arrays (count_cases.site_cases): here the things the lists cannot say"""
    big = [c for c in CASES if c.kind == "site" and c.planes == 64]
    (ac, ns), (n_us, het, hom) = next(c for c in big if c.name == "site-64p-rot0").expected()
    assert int(hom.max()) == 64 and int(ac.max()) == 128, "all 64 planes on one bin: 64 homozygotes, 128 copies"
    assert int(het.max()) == 64
    more = next(c for c in CASES if c.name == "site-130p-rot0").expected()
    assert int(more[1][2].max()) == 130 and int(more[0][0].max()) == 260
    assert any(not np.array_equal(c.expected()[0][0].astype(np.int64), (c.expected()[1][1] + 2 * c.expected()[1][2]).astype(np.int64)) for c in big), \
        "no cell with exactly one stray index: the tags and the genotype counts never differ"


def test_every_seam_is_claimed():
    for kind, seams in cc.REQUIRED.items():
        assert len(set(seams)) == len(seams), kind
        claimed = {s: [c.name for c in CASES if c.kind == kind and s in c.seams] for s in seams}
        assert not [s for s in seams if not claimed[s]], kind
    print({kind: sum(c.kind == kind for c in CASES) for kind in cc.REQUIRED}, {kind: len(s) for kind, s in cc.REQUIRED.items()})


def test_the_full_cross_of_kinds_and_spots_stands_in_every_shape():
    K, S = len(cc.KIND_NAMES), len(cc.SAMPLE_SPOTS)
    assert (K, S) == (43, 9)
    for planes, n in cc.SAMPLE_SHAPES:
        mine = [c for c in CASES if c.kind == "sample" and c.name.startswith("sample-kinds-%dx%d" % (planes, n))]
        assert len(mine) == (1 if planes >= K else -(-K // planes))
        claimed = {s for c in mine for s in c.seams if s.startswith("kind-")}
        assert claimed == {"kind-%s@%s#%dx%d" % (k, s, planes, n) for k in cc.KIND_NAMES for s in cc.SAMPLE_SPOTS}
        assert all(len(c.directed) == (K * S if planes >= K else planes * S) for c in mine)


def test_the_derived_sizes():
    assert cc.pair_plan(cc.N_WORDS_17, cc.pair_tiles(17)) == (64, 342) and cc.N_WORDS_17 - 341 * 64 == 1 and cc.pair_tiles(17) == 3
    assert cc.sample_plan(cc.N_VARS_3, 3) == (512, 342) and cc.N_VARS_3 - 341 * 512 == 1


def test_pack_to_count():
    """the cells of the end-to-end run pack to planes that count to the written-down table, and stand on the seam words of the shape"""
    e = cc.pack_to_count()
    assert (e.run, e.n_runs) == (64, 1025) and e.n % 64 == 1 and (e.n + 63) // 64 == e.n_words
    planes = pack_plain(e.g1, e.g2, None, False, e.vao())
    assert planes.shape == (2, 3, e.n_words)
    assert np.array_equal(pair_words_plain(planes), e.expected())
    words = {r >> 6 for r in e.directed}
    assert words == {cc.trip_word(w, e.n_words, e.run, e.n_runs) for w in cc.TRIP_WORDS} and e.n - 1 in e.directed
    seen = set(e.directed.values())
    assert len(seen) >= 9 and any(None in ds for ds in seen)


def test_no_case_is_left_out_of_the_gpu_file():
    import test_gpu_count_edges as gpu
    ran = [c.name for cases in gpu.RUN.values() for c in cases]
    left_out = [c.name for c in CASES if c.name not in ran]
    print("%d cases, %d run on the device, %d left out" % (len(CASES), len(ran), len(left_out)))
    assert len(ran) == len(set(ran)) == len(CASES) and not left_out
    text = open(gpu.__file__).read()
    assert "skip" not in text and "xfail" not in text
