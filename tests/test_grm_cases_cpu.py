"""The case table of the genetic relationship matrix (tests/grm_cases.py), proved against the restatement (tests/grm_model.py) without a
GPU: every case does what it claims, so a device that equals the model over the table has met each edge."""
import numpy as np
import pytest

import grm_cases
import grm_model as M

CASES = grm_cases.directed_cases()
BY_NAME = {c["name"]: c for c in CASES}


def _table(c):
    return M.weights_table(c["D"], c["haploid"], c["maf_ppm"], c["min_n"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_case_does_what_it_claims(case):
    w = _table(case)
    if case["enters"] is not None:
        assert list(w[:, 3] == 1) == case["enters"]
    assert (np.abs(w[:, :3].astype(np.int64)) <= M.MAX_Q).all() and not w[w[:, 3] == 0].any()


def test_names_are_unique_and_every_listed_size_is_there():
    assert len(BY_NAME) == len(CASES)
    assert all("samples_%d" % s in BY_NAME for s in (1, 2, 15, 16, 17, 31, 33, 64, 65, 130))
    assert all("records_%d" % r in BY_NAME for r in (0, 1, 63, 64, 65, 4097))


def test_the_q_boundary_flips_between_508_and_509():
    w = _table(BY_NAME["q_boundary_508_enters"])
    assert tuple(w[0, :3]) == BY_NAME["q_boundary_508_enters"]["q_first"] and w[0, 2] == 32608
    assert tuple(w[1, :3]) == (-32608, -16272, 64), "the mirrored record"
    flips = [bool(M.weights_table(grm_cases._one_alt(n).reshape(1, -1))[0, 3]) for n in range(500, 520)]
    assert flips == [n <= 508 for n in range(500, 520)], "both sides exist, and the flip is where the issue puts it"
    q, enters = M.weights_from_counts(508, 0, 1)
    assert int(q[2]) == 32640 and not enters, "509 samples: one beyond MG_GRM_MAX_Q"


def test_maf_and_min_n_are_at_equality():
    c = BY_NAME["maf_at_and_below"]
    n0, n1, n2 = M.counts_from_dosage(c["D"])
    ac, an = n1 + 2 * n2, 2 * (n0 + n1 + n2)
    minor = np.minimum(ac, an - ac)
    assert list(minor * 1000000 - c["maf_ppm"] * an) == [0, -50000 * 200 // 10, 0, -50000 * 200 // 10, 0]
    c = BY_NAME["min_n_at_and_below"]
    assert list(sum(M.counts_from_dosage(c["D"]))) == [c["min_n"], c["min_n"] - 1, 40]


def test_digit_extremes_are_met():
    c = BY_NAME["digit_extremes"]
    h, l = M.digits(_table(c)[:, :3].astype(np.int64))
    assert (l[0] == 127).any() and (l[1] == -128).any()
    h, l = M.digits(_table(BY_NAME["q_boundary_508_enters"])[:, :3].astype(np.int64))
    assert h.max() == 127 and h.min() == -127, "h = -128 would need q <= -32641, which MG_GRM_MAX_Q refuses"
    q = np.arange(-M.MAX_Q, M.MAX_Q + 1)
    h, l = M.digits(q)
    assert (256 * h + l == q).all() and h.min() == -127 and h.max() == 127 and l.min() == -128 and l.max() == 127


def test_haploid_weights():
    c = BY_NAME["haploid"]
    w = _table(c)
    D = np.where(c["D"] == 1, -1, c["D"])
    n0, _, n2 = M.counts_from_dosage(D)
    assert (c["D"][3, :5] == 1).all() and n0[3] + n2[3] == (c["D"][3] >= 0).sum() - 5, "the dosage-1 bits are ignored"
    p = n2 / (n0 + n2)
    ok = w[:, 3] == 1
    assert ok.sum() >= 30
    for d, x in ((0, 0.0), (2, 1.0)):                                              # (x - p) / sqrt(p (1 - p)), to half a unit of the fixed point
        assert np.abs(w[ok, d] / 1024.0 - (x - p[ok]) / np.sqrt(p[ok] * (1 - p[ok]))).max() <= 0.5 / 1024 + 1e-9
    assert _table(BY_NAME["haploid_maf_and_min_n"])[:, 3].sum() < ok.sum()


def test_diploid_weights_are_the_standardised_dosage():
    c = BY_NAME["samples_130"]
    w = _table(c)
    n0, n1, n2 = M.counts_from_dosage(c["D"])
    p = (n1 + 2 * n2) / (2 * (n0 + n1 + n2))
    ok = w[:, 3] == 1
    assert ok.sum() >= 40
    for d in range(3):
        assert np.abs(w[ok, d] / 1024.0 - (d - 2 * p[ok]) / np.sqrt(2 * p[ok] * (1 - p[ok]))).max() <= 0.5 / 1024 + 1e-9


@pytest.mark.parametrize("name", ["samples_1", "samples_2", "samples_17", "never_enter", "haploid", "multiallelic_among_biallelic", "records_65"])
def test_the_matrix_form_is_the_loop(name):
    c = BY_NAME[name]
    args = (c["D"], c["n_samples"], c["haploid"], c["maf_ppm"], c["min_n"])
    S, N, seen, entered = M.grm_sums(*args)
    S2, N2, seen2, entered2 = M.grm_sums_by_loop(*args)
    assert [int(x) for x in S] == S2 and [int(x) for x in N] == N2 and (seen, entered) == (seen2, entered2)
    X, Cc, _ = M.cell_weights(*args[:1], *args[2:])
    h, l = M.digits(X)
    a, b = M.pair_index(c["n_samples"])
    folded = 65536 * (h.T @ h) + 256 * (h.T @ l + l.T @ h) + l.T @ l
    assert np.array_equal(folded[a, b], S), "the five products fold to the sum"


def test_the_multiallelic_rows_count_nothing():
    c = BY_NAME["multiallelic_among_biallelic"]
    w = M.words_from_dosage(c["D"], c["n_samples"], spare_bits=False)
    assert not w[:, :, c["no_bits"]].any() and not _table(c)[c["no_bits"]].any()
    keep = [v for v in range(c["D"].shape[0]) if v not in c["no_bits"]]
    S, N, seen, entered = M.grm_sums(c["D"], 33)
    S2, N2, seen2, entered2 = M.grm_sums(c["D"][keep], 33)
    assert np.array_equal(S, S2) and np.array_equal(N, N2) and entered == entered2 and seen == seen2 + 2


def test_words_round_trip_and_spare_bits():
    from ibd_model import dosage_from_words
    c = BY_NAME["samples_130"]
    w = M.words_from_dosage(c["D"], 130)
    assert (w[2] >> np.uint64(2) == np.uint64((1 << 62) - 1)).all(), "the spare bits are set"
    clean = M.words_from_dosage(c["D"], 130, spare_bits=False)
    assert np.array_equal(dosage_from_words(clean, 130), c["D"])


def test_the_fold_case_passes_31_bits():
    D, records = grm_cases.fold_case()
    w = M.weights_table(D)
    h, _ = M.digits(w[0, :3].astype(np.int64))
    assert w[0, 3] == 1 and h[2] == 127 and 127 * 127 == 16129
    assert 16129 * 133144 < 2 ** 31 <= 16129 * 133145 <= 16129 * records
    S, N, _, _ = M.grm_sums(D, grm_cases.FOLD_SAMPLES)
    assert int(S[0]) == 32608 ** 2 and int(S[0]) * records < 2 ** 63


def test_text_value_rounds_half_away_from_zero():
    assert M.grm_text_value(0, 0) == "." and M.grm_text_value(0, 5) == "0.000000"
    assert M.grm_text_value(1 << 20, 1) == "1.000000" and M.grm_text_value(-(1 << 20), 1) == "-1.000000"
    assert M.grm_text_value(1 << 19, 1 << 6) == "0.007813" and M.grm_text_value(-(1 << 19), 1 << 6) == "-0.007813", "0.0078125: a tie"
    assert M.grm_text_value(-1, 4) == "0.000000", "a value that rounds to zero has no sign"
    assert M.grm_text_value(32608 ** 2, 1) == "1014.024414"


def test_maf_text():
    assert [M.parse_maf(t) for t in ("0.01", "0", "0.5", ".25", "0.000001", "0.123456", "0.")] == [10000, 0, 500000, 250000, 1, 123456, 0]
    assert [M.parse_maf(t) for t in ("0.5000001", "0.51", "1", "-0.1", "1e-2", "", ".", "0.1234567", "0,1", "00.1")] == [None] * 10


# ---- the plan cases: the Gram kernel without atomics and a full run of the i32 accumulators -------------------------------------------

PLAN_CASES = grm_cases.plan_cases()


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c["name"] for c in PLAN_CASES])
def test_a_plan_case_hits_the_plan_it_states(case):
    from test_grm_plan_cpu import step_plan
    assert step_plan(case["n_samples"], case["records"]) == case["plan"], "under the default cap of 384 MiB"
    assert sum(p[0] for p in case["plan"]) == case["records"] == case["count"] + (0 if case["front"] is None else len(case["front"]))
    atomics = [runs > 1 for _, _, runs in case["plan"]]
    assert all(atomics) if "atomics" in case["name"] and "no_atomics" not in case["name"] else not any(atomics)
    w = M.weights_table(case["record"].reshape(1, -1))
    assert w[0, 3] == 1, "the repeated record enters"
    if case["front"] is not None:
        F = case["front"]
        assert len(F) == grm_cases.FRONT_RECORDS and len({F[:, s].tobytes() for s in range(case["n_samples"])}) == case["n_samples"], "no two samples alike"
        assert M.weights_table(F)[:, 3].sum() >= 250


def test_the_plan_cases_name_both_forms_and_the_flip():
    plans = {(c["n_samples"], c["records"], c["front"] is not None): c["plan"] for c in PLAN_CASES}
    assert len(plans) == len(PLAN_CASES) == 6 and len({c["name"] for c in PLAN_CASES}) == 6
    for front in (False, True):
        assert plans[(2017, 1025, front)] == [(1025, 1088, 1)], "17 MFMA steps in one run: one more than any run of the older tests"
        assert plans[(2017, 65537, front)] == [(65536, 65536, 1), (1, 64, 1)], "1,024 steps, GRM_MAX_RUN exactly, then a piece of one step"
        assert plans[(2016, 65537, front)] == [(65537, 32832, 2)], "63 blocks: 2,016 on and above the diagonal, below GRM_FILL"


def test_the_bound_record_comes_closest_to_the_i32_bound():
    n = grm_cases.BOUND_SAMPLES
    row = grm_cases.bound_record(n)
    assert (row == 2).sum() == 4 and (row == 0).sum() == n - 4 and [int(s) for s in np.nonzero(row)[0]] == [0, 31, 32, 2016]
    w = M.weights_table(row.reshape(1, -1))
    assert tuple(int(x) for x in w[0]) == grm_cases.BOUND_Q + (1,) == (-65, 16211, 32487, 1)
    h, l = M.digits(w[0, :3].astype(np.int64))
    assert int(h[2]) == grm_cases.BOUND_H == 127 and int(l[2]) == -25
    assert 127 * 127 == 16129 and 16129 * 65536 == 1_057_030_144 < 2 ** 30
    # no entering record has a larger |h|: |q| <= MG_GRM_MAX_Q bounds it (test_digit_extremes_are_met), and among the records of 2,017
    # called samples with hom-alt and hom-ref cells alone, q2 falls as the hom-alt count grows: three or fewer do not enter
    q, enters = M.weights_from_counts(n - np.arange(1, 40), 0, np.arange(1, 40))
    assert list(enters[:4]) == [False, False, False, True] and (np.diff(q[:, 2]) < 0).all()
    hq, _ = M.digits(np.arange(-M.MAX_Q, M.MAX_Q + 1))
    assert np.abs(hq).max() == 127
    # the pairs of two hom-alt samples carry it, in the table as in the accumulators
    S1, N1, _, _ = M.grm_sums(row, n)
    a, b = M.pair_index(n)
    both = (row[a] == 2) & (row[b] == 2)
    assert both.sum() == 10 and (S1[both] == 32487 ** 2).all() and (N1 == 1).all()
    # the same record one sample fewer (the flip case) enters as well
    assert M.weights_table(grm_cases.bound_record(n - 1).reshape(1, -1))[0, 3] == 1


def test_a_plan_case_expects_the_models_table():
    """the one-record table times the count, on top of the front's: held against the model over the whole input with a count of 5; the
    products in doubles are the model's integer products, over a narrow cohort as a whole and over the rows of both ends of the wide one"""
    D70 = grm_cases.random_dosage(200, 70, seed=12)
    for got, want in zip(grm_cases.sums_in_doubles(D70, 70), M.grm_sums(D70, 70)):
        assert np.array_equal(got, want)
    case = next(c for c in PLAN_CASES if c["name"] == "no_atomics_17_steps_behind_random_records")
    n = case["n_samples"]
    case = dict(case, count=5, records=len(case["front"]) + 5)
    S, N, seen, entered = grm_cases.plan_case_expected(case)
    words = grm_cases.plan_case_words(case)
    assert words.shape == ((n + 63) // 64, 3, 305) and seen == 305
    D = np.concatenate([case["front"], np.repeat(case["record"].reshape(1, -1), case["count"], axis=0)])
    assert np.array_equal(words, M.words_from_dosage(D, n))
    X, Cc, entered2 = M.cell_weights(D)
    assert entered == entered2
    full, full_n = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    a, b = M.pair_index(n)
    full[a, b], full_n[a, b] = S, N.astype(np.int64)
    rows = list(range(0, 34)) + list(range(n - 3, n))
    for r in rows:                                                                 # (row r of the upper triangle, in the model's integers)
        assert np.array_equal((X[:, r:r + 1] * X[:, r:]).sum(axis=0), full[r, r:]) and np.array_equal((Cc[:, r:r + 1] * Cc[:, r:]).sum(axis=0), full_n[r, r:])
    off = full[0:32, 32:64]
    assert (off != off.T).sum() > 900, "a swapped row and column would show"
