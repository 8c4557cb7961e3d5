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


# ---- the seam cases ---------------------------------------------------------------------------------------------------------------------

SEAMS = ld_cases.seam_cases()


def _model_pairs(case, words):
    pairs, row_off = ld_pairs(words, case["chrom"], case["pos"], **case["params"])
    return [(int(p["i"]), int(p["j"])) for p in pairs], row_off


@pytest.mark.parametrize("case", SEAMS, ids=[c["name"] for c in SEAMS])
def test_a_seam_case_is_what_it_says(case):
    got, row_off = _model_pairs(case, case["words"])
    assert got == case["pairs"], "the emitted pairs are exactly the claimed ones"
    assert set(case["present"]) <= set(got) and case["present"]
    p = case["params"]
    for i, j, rule in case["absent"]:
        assert (i, j) not in got and rule in why_not(case["words"], case["chrom"], case["pos"], i, j, **p), (i, j, rule)
    # the decoys alone change nothing: the table without them gives the pairs that touch none of them
    plain, _ = _model_pairs(case, case["plain"])
    assert plain == [(i, j) for i, j in got if i not in case["decoys"] and j not in case["decoys"]]
    assert int(row_off[-1]) == len(got) and all(0 < cap < len(got) for cap in case["caps"])
    # every record but the named ones is monomorphic, in every group
    named = sorted({v for pair in case["pairs"] for v in pair} | set(case["decoys"]) | {v for i, j, _ in case["absent"] for v in (i, j) if v < case["words"].shape[2]})
    mono = np.ones(case["words"].shape[2], dtype=bool)
    mono[named] = False
    assert (case["words"][:, 0, mono] == ld_cases.ALL_ONES).all() and not case["words"][:, 1:, mono].any()


def test_the_seam_cases_claim_every_seam():
    by_name = {c["name"]: c for c in SEAMS}
    assert set().union(*(c["seams"] for c in SEAMS)) == ld_cases.LD_SEAMS
    place = ld_cases.tile_place
    # the windows: the last pair of the window sits in the slab and lane the name implies, for 65 .. 1023 in a slab behind the first
    for W in (63, 65, 127, 128, 129, 1023):
        c = by_name["window_%d" % W]
        assert c["params"]["window"] == W and (5, 5 + W) in c["present"] and (5, 5 + W + 1, "window") in c["absent"]
        assert place(5, 5 + W)[1:3] == ((W - 1) // 64, (W - 1) % 64) and ((W - 1) // 64 >= 1) == (W > 64)
        offs = {j - i for i, j in c["present"] if i == 5}
        assert offs >= {o for o in (64, 65, 128, 129) if o <= W} | {64 * k + 63 for k in range(16) if 64 * k + 63 <= W}
        # behind the first slab, `lane < window` in place of `s0 + lane < window` would keep the pair one beyond the window
        assert W < 64 or W % 64 < W
    c = by_name["rows_of_a_tile"]
    assert {i for i, _ in c["present"]} == {3, 4, 15, 16, 17, 31, 32} and {place(i, j)[3] for i, j in c["present"]} >= {0, 63, 64, 78}
    assert max(place(i, j)[3] for i, j in c["present"]) == ld_cases.LD_TILE + 62 < ld_cases.LD_JN
    c = by_name["partner_is_the_last_record"]
    assert c["words"].shape[2] - 1 == 39 and (10, 39) in c["present"] and 0 in {v for pair in c["pairs"] for v in pair}, "record 0 varies: what lies one past a row"
    c = by_name["last_tile_has_no_partner"]
    n = c["words"].shape[2]
    assert (n - 1) % ld_cases.LD_TILE == 0 and c["params"]["n_first"] == n, "the last tile's first partner is record n_vars"
    c = by_name["a_later_slab_starts_beyond_the_table"]
    assert 1 + 64 < c["words"].shape[2] <= 1 + 128 < c["params"]["window"]
    c = by_name["write_positions"]
    mine = [j - 5 for i, j in c["pairs"] if i == 5]
    assert [place(5, 5 + o)[1:3] for o in mine] == [(0, 0), (0, 31), (0, 32), (0, 63), (2, 0), (2, 31), (2, 32), (2, 63)]
    six = [j for i, j in c["pairs"] if i == 6]
    assert len(six) == len(mine) - 1 and 5 // ld_cases.LD_R == 6 // ld_cases.LD_R, "two records of one wave, eight pairs and seven"
    before = sum(1 for i, _ in c["pairs"] if i < 5)
    assert [cap - before for cap in c["caps"]] == [2, 6, 8], "inside the ballot of slab 0, inside that of slab 2, and between record 5 and 6"
    c = by_name["n_first_8193"]
    _, row_off = _model_pairs(c, c["words"])
    assert c["params"]["n_first"] == ld_cases.SCAN_CHUNK + 1 and [int(x) for x in row_off[[1, 8191, 8192, 8193]]] == [1, 1, 2, 3]
    for G, g in ((15, 0), (16, 15), (17, 15), (17, 16), (32, 31), (33, 16), (33, 31), (33, 32)):
        c = by_name["groups_%d_vary_in_%d" % (G, g)]
        assert c["words"].shape[0] == G and {grp for grp, _ in c["decoys"].values()} == {(g + 1) % G, (g - 1) % G}
        assert c["words"][g, 1:, 2].any() and not np.delete(c["words"][:, :, 2], g, axis=0).any()


@pytest.mark.parametrize("plane,record,dosage", ld_cases.pack_cases())
def test_a_pack_case_is_exactly_one_bit(plane, record, dosage):
    g1, g2, gq, vao = ld_cases.pack_case(plane, record, dosage)
    want = np.zeros((3, ld_cases.PACK_N), dtype=np.uint64)
    want[dosage, record] = np.uint64(1) << np.uint64(plane)
    assert np.array_equal(site_words(g1, g2, gq, False, vao, ld_cases.PACK_MIN_GQ), want)
    assert (site_words(g1, g2, gq, False, vao, ld_cases.PACK_MIN_GQ - 1)[2] == ld_cases.ALL_ONES).sum() >= ld_cases.PACK_N - 1, "one below the mask every decoy is a cell"
    assert {p for p, _, _ in ld_cases.pack_cases()} == {0, 3, 4, 5, 62, 63} and {v for _, v, _ in ld_cases.pack_cases()} == {0, 63, 64, ld_cases.PACK_N - 1}
    assert {d for _, _, d in ld_cases.pack_cases()} == {0, 1, 2}


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


def test_the_gpu_file_runs_every_seam_case_of_the_three_tables():
    import grm_cases
    import ibd_cases
    import test_gpu_site_word_edges as gpu
    assert [c["name"] for c in gpu.LD_SEAMS] == [c["name"] for c in SEAMS]
    assert [c["name"] for c in gpu.IBD_SEAMS] == [c["name"] for c in ibd_cases.seam_cases()]
    assert [c["name"] for c in gpu.GRM_PLANS] == [c["name"] for c in grm_cases.plan_cases()]
    text = open(gpu.__file__).read()
    assert "ld_cases.pack_cases()" in text and "ibd_cases.TR_SAMPLES" in text and "ibd_cases.TR_RECORDS" in text
    assert "skip" not in text and "xfail" not in text
    print("%d LD, %d pack, %d IBD, %d transpose and %d GRM cases run on the device" % (len(gpu.LD_SEAMS), len(ld_cases.pack_cases()), len(gpu.IBD_SEAMS),
                                                                                   len(ibd_cases.TR_SAMPLES) * len(ibd_cases.TR_RECORDS), len(gpu.GRM_PLANS)))
