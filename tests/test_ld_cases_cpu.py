"""The LD case table (tests/ld_cases.py) is what it says it is, and the restatement (tests/ld_model.py) agrees with itself: the matrix
form of ld_pairs against the popcount form of pair_value, pair by pair.  No GPU."""
import numpy as np
import pytest

import ld_cases
import ld_model
from malva_amd.capi import EXPORTED, LD_MAX_GROUPS, LD_MAX_WINDOW, LD_PAIR
from ld_model import RULES, dosage_from_words, ld_pairs, pair_value, site_words, why_not, words_from_dosage

CASES = ld_cases.directed_cases()


def test_the_model_speaks_of_the_abi_as_it_is():
    """the five calls are exported, the pair is the model's 24 bytes, the limits are the header's"""
    import os
    import re
    assert {"mg_pack_site_dosage", "mg_pack_site_dosage_device", "mg_ld_window", "mg_ld_window_device", "mg_ld_stats"} <= set(EXPORTED)
    assert LD_PAIR == ld_model.LD_PAIR and LD_PAIR.itemsize == 24
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "malva_hip.h")).read()
    assert int(re.search(r"#define MG_LD_MAX_GROUPS (\d+)", header).group(1)) == LD_MAX_GROUPS == 256
    assert int(re.search(r"#define MG_LD_MAX_WINDOW (\d+)", header).group(1)) == LD_MAX_WINDOW == 1024
    assert max(len(ld_cases.group_sizes_for(g)) for g in ld_cases.GROUPS) == LD_MAX_GROUPS and max(ld_cases.WINDOWS) == LD_MAX_WINDOW


def _emitted(case):
    pairs, row_off = ld_pairs(case["words"], case["chrom"], case["pos"], **case["params"])
    return {(int(p["i"]), int(p["j"])): p for p in pairs}, row_off


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_a_directed_case_is_what_it_says(case):
    i, j = case["pair"]
    got, row_off = _emitted(case)
    why = why_not(case["words"], case["chrom"], case["pos"], i, j, **case["params"])
    assert why <= set(RULES)
    if case["says"] == "emitted":
        assert not why and (i, j) in got
        n, cov, vx, vy, r2 = pair_value(case["words"], i, j)
        p = got[(i, j)]
        assert (int(p["n"]), int(p["sign"]), float(p["r2"])) == (n, (cov > 0) - (cov < 0), r2)
        if case["sign"] is not None:
            assert int(p["sign"]) == case["sign"]
    else:
        assert why == {case["says"]}, "rejected by that rule and by no other"
        assert (i, j) not in got
    assert int(row_off[-1]) == len(got)


def test_every_rule_and_every_sign_has_a_case():
    says = {c["says"] for c in CASES}
    assert says >= {"emitted", "vx", "vy", "min_n", "chrom", "max_bp", "window", "n_first", "min_r2"}
    assert {c["sign"] for c in CASES} >= {-1, 0, 1}


def test_the_wide_case_rounds_both_conversions():
    case = CASES[0]
    assert case["words"].shape[0] == 256
    n, cov, vx, vy, r2 = pair_value(case["words"], 0, 1)
    num, den = cov * cov, vx * vy
    assert n > 15000 and max(abs(cov), vx, vy) <= 1 << 30
    for x in (num, den):
        assert x > 1 << 53 and int(float(x)) != x, "beyond 2^53 and not representable"
    assert r2 == float(num) / float(den) and 0.2 <= r2 < 1.0


def test_the_matrix_form_rounds_as_python_ints_do():
    """a table of 16,384 samples: the products lie beyond 2^53, and several are no doubles"""
    D = np.concatenate([ld_cases.big_dosage(), ld_cases.random_dosage(10, 16384, 4, seed=9)])
    words = words_from_dosage(D)
    pairs, _ = ld_pairs(words, np.zeros(12, dtype=np.uint32), np.arange(12, dtype=np.uint32), 12, 11, 0, 1, 0.0)
    assert len(pairs) > 30
    beyond = 0
    for p in pairs:
        n, cov, vx, vy, r2 = pair_value(words, int(p["i"]), int(p["j"]))
        assert (int(p["n"]), float(p["r2"])) == (n, r2)
        beyond += vx * vy > 1 << 53 and int(float(vx * vy)) != vx * vy
    assert beyond >= 5


def test_the_threshold_cases_sit_on_the_threshold():
    exact, ulp = CASES[1], CASES[3]
    assert pair_value(exact["words"], 0, 1)[4] == 0.25 == exact["params"]["min_r2"]
    r2 = pair_value(ulp["words"], 0, 1)[4]
    assert ulp["params"]["min_r2"] == np.nextafter(r2, 2.0) and CASES[2]["params"]["min_r2"] == r2


@pytest.fixture(scope="module")
def random_tables():
    out = []
    for window, n_vars, n_groups in ((1, 257, 1), (3, 69, 2), (64, 130, 3), (64, 257, 256), (1024, 1090, 2)):
        words, chrom, pos, max_bp = ld_cases.window_case(window, n_vars, n_groups)
        out.append((window, words, chrom, pos, max_bp))
    return out


def test_random_tables_exercise_both_branches_at_min_r2(random_tables):
    defined = emitted = 0
    for window, words, chrom, pos, _ in random_tables:
        n = words.shape[2]
        defined += len(ld_pairs(words, chrom, pos, n, window, 0, 1, 0.0)[0])
        emitted += len(ld_pairs(words, chrom, pos, n, window, 0, 1, 0.2)[0])
    assert defined > 10000 and 0.1 * defined <= emitted <= 0.9 * defined, (defined, emitted)


def test_random_tables_have_what_the_gpu_test_counts_on(random_tables):
    for window, words, chrom, pos, max_bp in random_tables:
        n = words.shape[2]
        assert len(set(chrom.tolist())) == 4 and (np.bincount(chrom) == 1).any(), "several contigs, one of a single record"
        free, cut = ld_pairs(words, chrom, pos, n, window, 0, 1, 0.0)[0], ld_pairs(words, chrom, pos, n, window, max_bp, 1, 0.0)[0]
        assert 0 < len(cut) < len(free), "max_bp cuts windows"
        assert {-1, 0, 1} >= set(free["sign"].tolist()) >= {-1, 1}
        empty = ~np.bitwise_or.reduce(words, axis=(0, 1)).astype(bool)
        assert empty.any() and not np.isin(free["i"], np.nonzero(empty)[0]).any(), "records without cells, in no pair"


def test_matrix_form_equals_popcount_form(random_tables):
    window, words, chrom, pos, max_bp = random_tables[2]
    n = words.shape[2]
    pairs, row_off = ld_pairs(words, chrom, pos, n - 5, window, max_bp, 3, 0.1, block=7)
    want = []
    for i in range(n - 5):
        for j in range(i + 1, min(n, i + window + 1)):
            if not why_not(words, chrom, pos, i, j, n - 5, window, max_bp, 3, 0.1):
                nn, cov, vx, vy, r2 = pair_value(words, i, j)
                want.append((i, j, nn, (cov > 0) - (cov < 0), r2))
    assert [tuple(p) for p in pairs.tolist()] == want
    assert [int(x) for x in row_off] == [sum(1 for w in want if w[0] < i) for i in range(n - 4)]
    again, off2 = ld_pairs(words, chrom, pos, n - 5, window, max_bp, 3, 0.1)
    assert again.tobytes() == pairs.tobytes() and np.array_equal(off2, row_off), "the block size changes nothing"


def test_group_cut_changes_nothing():
    D = ld_cases.random_dosage(90, 70, 8, seed=5)
    chrom, pos = np.zeros(90, dtype=np.uint32), np.arange(90, dtype=np.uint32)
    one = ld_pairs(words_from_dosage(D, [64, 6]), chrom, pos, 90, 16, 0, 2, 0.2)
    for sizes in ([35, 35], [1] * 70, [6, 64]):
        other = ld_pairs(words_from_dosage(D, sizes), chrom, pos, 90, 16, 0, 2, 0.2)
        assert other[0].tobytes() == one[0].tobytes() and np.array_equal(other[1], one[1])


def test_site_words_by_hand():
    """records of 2, 1, 3 and 2 alleles; stray indexes -1 and A; the mask; haploid as a homozygote"""
    vao = np.array([0, 2, 3, 6, 8], dtype=np.uint32)
    g1 = np.array([[0, 0, 1, 1], [1, 0, 0, -1], [1, 0, 2, 2]], dtype=np.int32)
    g2 = np.array([[1, 0, 1, 1], [1, 0, 0, 0], [0, 0, 0, 1]], dtype=np.int32)
    gq = np.array([[40, 40, 40, 10], [40, 40, 40, 40], [10, 40, 40, 40]], dtype=np.int32)
    w = site_words(g1, g2, gq, False, vao, None)
    assert w.tolist() == [[0, 0, 0, 0], [0b101, 0, 0, 0], [0b010, 0, 0, 0b001]]
    w = site_words(g1, g2, gq, False, vao, 30)
    assert w.tolist() == [[0, 0, 0, 0], [0b001, 0, 0, 0], [0b010, 0, 0, 0]]
    w = site_words(g1, None, gq, True, vao, None)
    assert w.tolist() == [[0b001, 0, 0, 0], [0, 0, 0, 0], [0b110, 0, 0, 0b001]]
    V, X = dosage_from_words(w[None])
    assert V.shape == (4, 3) and X[0].tolist() == [0, 2, 2]
