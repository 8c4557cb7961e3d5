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
