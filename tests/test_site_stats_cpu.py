"""The restatement behind `call --cohort --site-stats` (tests/site_stats_model.py) checked on its own: the exact test against rational
arithmetic, directed values, the counting identity, the text rules."""
import math
from fractions import Fraction

import numpy as np

from site_stats_model import HEADER, af_text, geno_counts_plain, hwe_exact, site_stats_text

FACT = [math.factorial(i) for i in range(42)]


def hwe_rational(n, het, hom):
    """-> (hwe, exc_het, tied): the test in fractions.  The weight of h heterozygotes among n individuals with na copies of the allele is
    n! 2^h / (a! h! c!), a = (na - h) / 2 and c = (2 n - na - h) / 2 the two kinds of homozygotes.  tied: another count weighs exactly
    what the observed one does."""
    na = het + 2 * hom
    nb = 2 * n - na
    w = {h: Fraction(FACT[n] << h, FACT[(na - h) // 2] * FACT[h] * FACT[(nb - h) // 2]) for h in range(na & 1, min(na, nb) + 1, 2)}
    total = sum(w.values())
    tied = any(h != het and x == w[het] for h, x in w.items())
    return sum(x for x in w.values() if x <= w[het]) / total, sum(x for h, x in w.items() if h >= het) / total, tied


def test_the_model_against_rational_arithmetic():
    """every (n, het, hom) with n <= 40.  At most 41 terms, each at most 20 steps of 2 roundings of 2^-53, and the sums: below 1e-14,
    so 1e-12 leaves two orders of margin.  Where another term ties exactly with the observed one, rounding decides on which side of
    `<=` it falls: those cases are skipped for HWE (not for EXC_HET), and must stay below 1 %."""
    cases = skipped = 0
    worst = 0.0
    for n in range(41):
        for het in range(n + 1):
            for hom in range(n - het + 1):
                cases += 1
                p, e = hwe_exact(n, het, hom)
                want_p, want_e, tied = hwe_rational(n, het, hom)
                assert 0 < e <= 1 and 0 < p <= 1
                d = abs(Fraction(e) - want_e) / want_e
                worst = max(worst, float(d))
                assert d <= Fraction(1, 10 ** 12), (n, het, hom, e, float(want_e))
                if tied:
                    skipped += 1
                    continue
                d = abs(Fraction(p) - want_p) / want_p
                worst = max(worst, float(d))
                assert d <= Fraction(1, 10 ** 12), (n, het, hom, p, float(want_p))
    print("cases %d, skipped for a tie %d, worst relative difference %.3g" % (cases, skipped, worst))
    assert cases == 12341 and skipped < cases / 100


def test_directed_values():
    assert hwe_exact(0, 0, 0) == (1.0, 1.0)
    assert hwe_exact(1, 1, 0) == (1.0, 1.0)
    p, e = hwe_exact(3, 3, 0)
    assert abs(p - 0.4) < 1e-15 and abs(e - 0.4) < 1e-15
    p, e = hwe_exact(100, 21, 4)
    assert "%.6g" % p == "0.119447" and "%.6g" % e == "0.970068"
    assert hwe_exact(16384, 16384, 0) == (0.0, 0.0)                                # every heterozygous: the term underflows
    assert all(math.isnan(x) for x in hwe_exact(2, 1, 2))
    assert all(math.isnan(x) for x in hwe_exact((1 << 24) + 1, 0, 0))
    assert hwe_exact(1 << 24, 0, 0) == (1.0, 1.0)
    assert hwe_exact(50, 0, 0) == (1.0, 1.0) and hwe_exact(50, 0, 50) == (1.0, 1.0)  # one allele alone: one term
    p, e = hwe_exact(1000, 0, 20)                                                  # no heterozygote among 40 copies
    assert 0 < p < 1e-30 and e == 1.0
    assert hwe_exact(10, 3, 2) == hwe_exact(10, 3, 5)                              # the other allele's view: the same r and het


def _cells(planes, A, seed):
    rng = np.random.default_rng(seed)
    A = np.asarray(A)
    n = len(A)
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)
    g1, g2 = (rng.integers(-1, A[None, :] + 1, size=(planes, n)).astype(np.int32) for _ in range(2))
    gq = rng.integers(0, 60, size=(planes, n)).astype(np.int32)
    return g1, g2, gq, vao


def test_the_counts_add_up_per_record():
    g1, g2, gq, vao = _cells(37, [1, 2, 2, 3, 9, 2, 70, 2], seed=3)
    for min_gq in (None, 30):
        n, het, hom = geno_counts_plain(g1, g2, gq, False, vao, min_gq)
        for v in range(len(vao) - 1):
            s = slice(int(vao[v]), int(vao[v + 1]))
            assert int(het[s].sum()) + 2 * int(hom[s].sum()) == 2 * int(n[v])
            assert int(het[s].sum()) % 2 == 0
        hn, hhet, hhom = geno_counts_plain(g1, None, gq, True, vao, min_gq)
        assert not hhet.any()
        for v in range(len(vao) - 1):
            assert int(hhom[vao[v]:vao[v + 1]].sum()) == int(hn[v])
    full = geno_counts_plain(g1, g2, gq, False, vao)[0]
    assert (geno_counts_plain(g1, g2, gq, False, vao, 30)[0] <= full).all() and 0 < full.max() <= 37
    # by hand: record of 2 alleles; cells 0/0, 0/1, 1/1, 1/0, -1/0, 0/2, masked 1/1
    g1 = np.array([[0], [0], [1], [1], [-1], [0], [1]])
    g2 = np.array([[0], [1], [1], [0], [0], [2], [1]])
    gq = np.array([[9], [9], [9], [9], [9], [9], [1]])
    n, het, hom = geno_counts_plain(g1, g2, gq, False, [0, 2], 5)
    assert (int(n[0]), het.tolist(), hom.tolist()) == (4, [2, 2], [1, 1])


def test_the_text_rules():
    assert [af_text(*x) for x in ((0, 0), (0, 4), (4, 4), (1, 4), (2, 3), (1, 3), (1, 2000000), (1, 2000001), (999999, 1000000), (1999999, 2000000))] == \
        [".", "0", "1", "0.25", "0.666667", "0.333333", "0.000001", "0", "0.999999", "1"]
    cols = ["c1\t5\t.\tA\tC", "c1\t9\trs1\tAT\tA,ATT", "c2\t1\t.\tG\t.", "c2\t2\t.\tG\tT"]
    vao = [0, 2, 5, 6, 8]
    n = [100, 3, 7, 0]
    het = [21, 21, 3, 1, 2, 0, 0, 0]
    hom = [75, 4, 0, 1, 0, 7, 0, 0]
    text = site_stats_text(cols, 120, False, vao, n, het, hom)
    assert text == HEADER + \
        "c1\t5\t.\tA\tC\t120\t100\t200\t29\t0.145\t4\t21\t0.119447\t0.970068\n" \
        "c1\t9\trs1\tAT\tA,ATT\t120\t3\t6\t3,2\t0.5,0.333333\t1,0\t1,2\t1,1\t1,0.8\n" \
        "c2\t2\t.\tG\tT\t120\t0\t0\t0\t.\t0\t0\t.\t.\n"
    hap = site_stats_text(cols, 120, True, vao, n, [0] * 8, hom)
    assert hap == HEADER + \
        "c1\t5\t.\tA\tC\t120\t100\t100\t4\t0.04\t4\t0\t.\t.\n" \
        "c1\t9\trs1\tAT\tA,ATT\t120\t3\t3\t1,0\t0.333333,0\t1,0\t0,0\t.,.\t.,.\n" \
        "c2\t2\t.\tG\tT\t120\t0\t0\t0\t.\t0\t0\t.\t.\n"
    assert HEADER.rstrip("\n").split("\t") == "#CHROM POS ID REF ALT SAMPLES N AN AC AF HOM HET HWE EXC_HET".split()
