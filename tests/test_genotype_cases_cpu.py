"""The inputs of tests/test_gpu_genotype_edges.py hold what they claim -- asserted with the oracle alone, on any machine, so a
GPU test cannot pass because its inputs went soft.  The class letters are those of tests/geno_cases.py."""
import numpy as np
import pytest

import geno_cases as gc

SMALLEST_NORMAL = 2.2250738585072014e-308


def _values(exp, v):
    return exp.norm[int(exp.goff[v]):int(exp.goff[v + 1])]


def test_inputs_stay_below_2_30():
    cases = [gc.biallelic(257, False, 357), gc.many_alleles(True, 0.01, 0), gc.logf_specials(False), gc.logf_sweep(True),
             gc.mixed(0.5, False), gc.at_max_cov(59, True), gc.tiny(False)] + [c for _, c in gc.beyond_ln_table()]
    for c in cases:
        assert c.cov.dtype == np.uint32 and c.freq.dtype == np.float32 and c.var_allele_off.dtype == np.uint32
        assert int(c.cov.max()) < 1 << 30 and max(int(r[0].astype(np.int64).sum()) for r in gc.records(c)) < 1 << 30


# ---- A ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("haploid", [False, True])
def test_a_biallelic_waves_keep_forty_voters(haploid):
    for n in gc.BIALLELIC_COUNTS:
        case = gc.biallelic(n, haploid, 100 + n)
        assert np.all(np.diff(case.var_allele_off.astype(np.int64)) == 2) and len(case.var_allele_off) == n + 1
        assert int(case.cov.max()) > 200 or n < 63
        exp = gc.expected(case)
        for w in range(n // gc.WAVE):
            assert int(np.sum(exp.status[w * gc.WAVE:(w + 1) * gc.WAVE] == gc.ST_NORMAL)) >= 40, (n, w)
        if n >= 63:     # lanes that leave before the vote, of both kinds
            assert (exp.status == gc.ST_OVERCOV).any() and (exp.status == gc.ST_NOCOV).any()


@pytest.mark.parametrize("haploid", [False, True])
def test_a_the_odd_lane_votes_and_changes_nothing_else(haploid):
    plain = gc.biallelic(257, haploid, 357)
    pe = gc.expected(plain)
    for lane in gc.ODD_LANES:
        odd = gc.WAVE + lane
        case = gc.biallelic(257, haploid, 357, odd=odd)
        A = np.diff(case.var_allele_off.astype(np.int64))
        assert A[odd] == 3 and int(np.sum(A == 2)) == 256
        exp = gc.expected(case)
        assert exp.status[odd] == gc.ST_NORMAL
        for w in range(4):
            assert int(np.sum(exp.status[w * gc.WAVE:(w + 1) * gc.WAVE] == gc.ST_NORMAL)) >= 40
        keep = np.arange(257) != odd
        assert np.array_equal(exp.status[keep], pe.status[keep]) and np.array_equal(exp.gq[keep], pe.gq[keep])
        for v in np.nonzero(keep)[0]:
            assert np.array_equal(_values(exp, v), _values(pe, v), equal_nan=True)


def test_a_results_feel_a_reordered_sum():
    """a fast path that added its values in another order, or took the last quotient as the rest to 1, would differ from the oracle"""
    exp = gc.expected(gc.biallelic(257, False, 357))
    r = exp.raw.reshape(-1, 3)[exp.status == gc.ST_NORMAL]
    assert int(np.sum((r[:, 0] + r[:, 1]) + r[:, 2] != (r[:, 0] + r[:, 2]) + r[:, 1])) >= 10
    exp = gc.expected(gc.biallelic(257, True, 357))
    q = exp.norm.reshape(-1, 2)[exp.status == gc.ST_NORMAL]
    assert int(np.sum(q[:, 1] != 1.0 - q[:, 0])) >= 10


# ---- B ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("haploid", [False, True])
@pytest.mark.parametrize("rate", [0.001, 0.01])
def test_b_many_alleles_have_values_to_compare(haploid, rate):
    case = gc.many_alleles(haploid, rate, 0)
    A = np.diff(case.var_allele_off.astype(np.int64))
    want = gc.MANY_HAPLOID if haploid else gc.MANY_DIPLOID
    assert sorted(A[A > 2]) == list(want) and int(np.sum(A == 2)) >= 3
    assert min(want) < gc.EPS_TABLE <= sorted(want)[1]
    exp = gc.expected(case)
    assert np.all(exp.status == gc.ST_NORMAL)
    for v in np.nonzero(A > 2)[0]:
        c = case.cov[case.var_allele_off[v]:case.var_allele_off[v + 1]]
        assert int(c.max()) <= 3 and 20 <= int(c.sum()) <= 60
        q = _values(exp, v)
        assert len(q) == (A[v] if haploid else A[v] * (A[v] + 1) // 2)
        assert int(np.sum((q > 0) & (q != 1))) >= 2, v


# ---- C ---------------------------------------------------------------------------------------------------------------
def test_c_beyond_the_ln_table():
    families = gc.beyond_ln_table()
    assert [n for n, _ in families] == ["thirds", "skewed", "halves"]
    for name, case in families:
        assert case.max_cov == 1 << 20 and 0.29 < case.error_rate <= 0.5
        exp = gc.expected(case)
        assert np.all(exp.status == gc.ST_NORMAL)
        big = gc.beyond_table(case)
        totals = np.array([int(c.astype(np.int64).sum()) for c, _ in gc.records(case)])
        assert int(big.sum()) >= 30 and int((~big).sum()) >= 20
        assert {65535, 65536, 65537} <= set(totals.tolist()) and totals.max() >= (300000 if name == "skewed" else 1000000)
        strong = 0
        for v, (c, _) in enumerate(gc.records(case)):
            q = _values(exp, v)
            assert int(np.sum((q > 1e-3) & (q < 1 - 1e-3))) >= 2, (name, v)
            b = float(np.max(q)) * 100
            assert abs(b - np.floor(b) - 0.5) > 1e-6, (name, v)
            if big[v]:
                # two live genotypes whose log_binomial arguments at or beyond the table's end are not the same ones in the same order
                c = c.astype(np.int64)
                live = np.nonzero(q > 1e-3)[0]
                if case.haploid:
                    args = {(int(c[g]), int(totals[v] - c[g])) for g in live}
                else:
                    pairs = [(i, j) for i in range(3) for j in range(i, 3)]
                    args = {(int(c[pairs[g][0]] + c[pairs[g][1]]), int(c[pairs[g][0]])) for g in live if pairs[g][0] != pairs[g][1]}
                assert len(args) >= 2 or name == "skewed" and v == 0, (name, v)
                strong += len({a for a in args if min(a) >= gc.LN_TABLE} if case.haploid else {a[0] for a in args if a[0] >= gc.LN_TABLE}) >= 2
        # ... and in these, two live genotypes each have an argument of their own at or beyond 65536.  Not every record can: one
        # whose total straddles 65536 has pair sums below it (there ln(total) alone leaves the table, and it is common to all
        # genotypes), and skewed record 0 is the symmetric (40000, 30000, 30000), whose two live genotypes take the same ones.
        # In `halves` the two genotypes take ln(c0) and ln(c1) in swapped order -- with two alleles and one ploidy there is no
        # other pair -- so a wrong ln shows there only through rounding; `thirds` and `skewed` carry the stronger check.
        assert strong >= 15, name
    # the pair sums of one record sit on 65535, 65536 and 65537
    c = gc.records(families[0][1])[0][0].astype(np.int64)
    assert sorted([int(c[0] + c[1]), int(c[0] + c[2]), int(c[1] + c[2])]) == [65535, 65536, 65537]


def test_c_the_larger_sample_is_all_beyond_the_table():
    for name, case in gc.beyond_ln_sample():
        exp = gc.expected(case)
        assert 1500 <= len(exp.status) <= 5000 and np.all(exp.status == gc.ST_NORMAL) and gc.beyond_table(case).all()
        per = 2 if case.haploid else 6
        q = exp.norm.reshape(-1, per)
        assert np.all(np.sum((q > 1e-3) & (q < 1 - 1e-3), axis=1) >= 2), name
        b = q.max(axis=1) * 100
        assert np.all(np.abs(b - np.floor(b) - 0.5) > 1e-6), name
        totals = case.cov.reshape(-1, 2 if case.haploid else 3).astype(np.int64).sum(axis=1)
        assert totals.min() < 70000 and totals.max() > 900000


# ---- D ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("haploid", [False, True])
def test_d_every_logf_branch_is_taken(haploid):
    case = gc.logf_specials(haploid)
    exp = gc.expected(case)
    A = np.diff(case.var_allele_off.astype(np.int64))
    assert set(A.tolist()) == {2, 3}
    for x in (1e-40, 1e-45, float(gc.F32_MIN_NORMAL), 1.0, 1.5, -0.5, float("inf")):
        assert int(np.sum(case.freq == np.float32(x))) >= 4
    assert int(np.sum(np.isnan(case.freq))) >= 4 and np.float32(1e-45) > 0
    seen = {}
    for v, args in enumerate(gc.logf_args(case)):
        if exp.status[v] != gc.ST_NORMAL:
            continue
        for key in {(kind, gc.logf_branch(x)) for kind, x in args}:
            seen[key] = seen.get(key, 0) + 1
    for b in gc.LOGF_BRANCHES_FREQ:
        if b != "zero":
            assert seen.get(("freq", b), 0) >= 4, b
    if not haploid:
        for b in gc.LOGF_BRANCHES_PAIR:
            assert seen.get(("pair", b), 0) >= 4, b
    # the special values do not drown every record: some keep a call
    assert int(np.sum(exp.gq > 0)) >= 40


@pytest.mark.parametrize("haploid", [False, True])
def test_d_the_sweep_visits_all_sixteen_intervals(haploid):
    case = gc.logf_sweep(haploid)
    exp = gc.expected(case)
    assert len(exp.status) == 128 and np.all(exp.status == gc.ST_NORMAL)
    hits = np.zeros(16, dtype=np.int64)
    for args in gc.logf_args(case):
        xs = [x for kind, x in args if kind == ("freq" if haploid else "pair")]
        x = xs[-1]                                  # the swept frequency / the one pair product
        assert gc.logf_branch(x) in ("normal", "above_one")
        if not haploid:
            assert np.float32(x) == args[1][1]      # 2 * 0.5 * f is f
        hits[gc.logf_interval(x)] += 1
    assert np.all(hits == 8)
    assert not np.isnan(exp.norm).any() and len(set(exp.gq.tolist())) > 3


# ---- E ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("haploid", [False, True])
def test_e_rates_and_max_cov(haploid):
    base = gc.mixed(0.001, haploid)
    for rate in gc.RATES:
        case = gc.mixed(rate, haploid)
        assert np.array_equal(case.cov, base.cov) and np.array_equal(case.freq, base.freq) and case.error_rate == rate
        exp = gc.expected(case)
        assert 450 <= len(exp.status) <= 550
        assert int(np.sum(exp.status == gc.ST_NORMAL)) >= 300 and (exp.status == gc.ST_OVERCOV).any() and (exp.status == gc.ST_NOCOV).any()
        if rate in (0.01, 0.5):
            assert int(np.sum(exp.gq > 0)) >= 300
        if rate == 1e-8:
            assert np.float32(1) - np.float32(rate) == 1 and int(np.sum(exp.gq > 0)) >= 100     # c_hom is 0
    for mc in gc.MAX_COVS:
        case = gc.at_max_cov(mc, haploid)
        assert case.max_cov == mc and int(case.cov.max()) <= 61
        exp = gc.expected(case)
        top = np.array([int(c.max()) for c, _ in gc.records(case)])
        at, above = top == mc, top == mc + 1
        assert int(at.sum()) >= 50 and int(above.sum()) >= 50
        assert np.all(exp.status[at] == (gc.ST_NORMAL if mc else gc.ST_NOCOV)) and np.all(exp.status[above] == gc.ST_OVERCOV)
        assert np.all(exp.gq[above] == 0)
        if mc:
            assert int(np.sum(exp.gq[at] > 0)) >= 50


# ---- F ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("haploid", [False, True])
def test_f_three_hundred_records_of_subnormal_values(haploid):
    case = gc.tiny(haploid)
    exp = gc.expected(case)
    assert len(exp.status) <= 5000
    t = gc.all_tiny(exp)
    assert int(t.sum()) >= 300
    # and they are not all one record: the normalised values differ from record to record
    assert len({tuple(_values(exp, v)) for v in np.nonzero(t)[0]}) >= 100
    if haploid:
        v = [i for i, (c, _) in enumerate(gc.records(case)) if list(c) == [54, 54, 54]][0]
        r = exp.raw[int(exp.goff[v]):int(exp.goff[v + 1])]
        assert t[v] and np.all(r == r[0]) and 1.96e-313 < r[0] < 1.97e-313 < SMALLEST_NORMAL
