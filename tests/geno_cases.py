"""Inputs that drive the genotype kernel (csrc/geno_dev.h) into the branches the random tests do not reach, and what the
oracle says of them.  No GPU and no HIP here: tests/test_genotype_cases_cpu.py checks on any machine that every class
holds what it claims, tests/test_gpu_genotype_edges.py hands the same arrays to the device.

A case is (cov u32, freq f32, var_allele_off u32, error_rate, max_cov, haploid): the arguments of Context.genotype.
Every coverage and every total stays below 2^30 (the reference casts them to int)."""
from collections import namedtuple

import numpy as np

from oracle import capi as ocapi

Case = namedtuple("Case", "cov freq var_allele_off error_rate max_cov haploid")
Expected = namedtuple("Expected", "g1 g2 gq status norm raw goff")

WAVE = 64                      # lanes of a wave: record v of a call is lane v % 64 of wave v // 64
LN_TABLE = 65536               # MG_LN_TABLE: ln(n) comes from the host-filled table for n < this
EPS_TABLE = 256                # MG_EPS_TABLE: the per-allele-count floats come from the host-filled table for A < this
ST_NORMAL, ST_OVERCOV, ST_ONE, ST_NOCOV = 0, 1, 2, 3
F32_MIN_NORMAL = np.float32(1.17549435e-38)
THIRD = float(np.float32(1.0) / np.float32(3.0))


def pack(records, error_rate, max_cov, haploid):
    """[(coverages, frequencies)] -> Case"""
    off = np.zeros(len(records) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(c) for c, _ in records])
    cov = np.concatenate([np.asarray(c, dtype=np.int64) for c, _ in records])
    assert cov.min() >= 0 and cov.max() < 1 << 30
    with np.errstate(all="ignore"):
        freq = np.concatenate([np.asarray(f, dtype=np.float32) for _, f in records])
    assert len(cov) == len(freq) == off[-1]
    return Case(cov.astype(np.uint32), freq, off, error_rate, max_cov, bool(haploid))


def records(case):
    o = case.var_allele_off
    return [(case.cov[o[v]:o[v + 1]], case.freq[o[v]:o[v + 1]]) for v in range(len(o) - 1)]


def status_of(cov, max_cov):
    cov = np.asarray(cov, dtype=np.int64)
    assert int(cov.sum()) < 1 << 30
    if (cov > max_cov).any():
        return ST_OVERCOV
    if len(cov) == 1:
        return ST_ONE
    return ST_NOCOV if cov.sum() == 0 else ST_NORMAL


def expected(case):
    """The oracle over a case, through the calls tests/test_gpu_genotype.py's _oracle_variant makes.  `norm` and `raw` are laid
    out as Context.genotype lays `probs` out (A or A (A + 1) / 2 values per record, offsets in `goff`); records whose status is
    not normal have NaN there and are not compared."""
    recs = records(case)
    n = len(recs)
    A = np.array([len(c) for c, _ in recs], dtype=np.int64)
    goff = np.zeros(n + 1, dtype=np.uint64)
    goff[1:] = np.cumsum(A if case.haploid else A * (A + 1) // 2)
    g1, g2, gq = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    st = np.zeros(n, np.uint8)
    norm = np.full(int(goff[-1]), np.nan)
    raw = np.full(int(goff[-1]), np.nan)
    for v, (c, f) in enumerate(recs):
        gts = ocapi.genotype(c, f, case.error_rate, case.max_cov, case.haploid)
        vals = np.array([g[2] for g in gts], dtype=np.float64)
        bi, q, nv = ocapi.select_gt(vals)
        g1[v], g2[v] = (gts[bi][0], gts[bi][1]) if bi >= 0 else (0, -1 if case.haploid else 0)
        gq[v] = q
        st[v] = status_of(c, case.max_cov)
        if st[v] == ST_NORMAL:
            a, b = int(goff[v]), int(goff[v + 1])
            assert len(vals) == b - a
            norm[a:b], raw[a:b] = nv, vals
    return Expected(g1, g2, gq, st, norm, raw, goff)


# ---- A: biallelic waves ---------------------------------------------------------------------------------------------
BIALLELIC_COUNTS = (1, 63, 64, 65, 129, 256, 257)
ODD_LANES = (0, 31, 63)


def biallelic(n, haploid, seed, odd=None):
    """n biallelic records, coverages 0..60 per allele (0..5 in three of ten), about 15 % of them over-covered or uncovered (those lanes leave before
    the wave votes).  Record `odd`, if given, gets a third allele and an ordinary coverage: its wave takes the general path.
    Every record is drawn from a stream of its own, so all records but `odd` are the same with and without it."""
    recs = []
    for v in range(n):
        rng = np.random.default_rng([seed, v])
        c = rng.integers(0, 61, size=2)
        f = rng.dirichlet(np.ones(2))
        u = rng.random()
        if u > 0.7:
            c = c % 6                  # a few reads: the two or three values are of one size and their sum feels its order
        if v == odd:
            c = np.append(np.maximum(c, 1), rng.integers(0, 61))
            f = rng.dirichlet(np.ones(3))
        elif u < 0.075:
            c[rng.integers(0, 2)] = 201 + rng.integers(0, 100)
        elif u < 0.15:
            c[:] = 0
        recs.append((c, f))
    return pack(recs, 0.001, 200, haploid)


# ---- B: allele counts around the end of the error-rate table ---------------------------------------------------------
MANY_HAPLOID = (255, 256, 257, 300)
MANY_DIPLOID = (255, 256, 257)


def many_alleles(haploid, error_rate, seed):
    """one record per allele count, coverages 0..3 and a total of 20..60, each between a few biallelic records"""
    rng = np.random.default_rng(seed)
    recs = []

    def small():
        recs.append((rng.integers(0, 40, size=2) + 1, rng.dirichlet(np.ones(2))))
    small()
    for A in (MANY_HAPLOID if haploid else MANY_DIPLOID):
        c = np.zeros(A, dtype=np.int64)
        for _ in range(int(rng.integers(20, 61))):
            a = int(rng.integers(0, A))
            while c[a] == 3:
                a = int(rng.integers(0, A))
            c[a] += 1
        recs.append((c, rng.dirichlet(np.ones(A))))
        small()
        small()
    return pack(recs, error_rate, 200, haploid)


# ---- C: ln(n) beyond the host table -----------------------------------------------------------------------------------
BIG_MAX_COV = 1 << 20


def _thirds(rng, n):
    """three coverages that add up to n, each within about sqrt(n) / 4 of n / 3"""
    d = np.rint(rng.normal(0, 0.25 * np.sqrt(n), size=2)).astype(np.int64)
    c0, c1 = n // 3 + d[0], n // 3 + d[1]
    return [c0, c1, n - c0 - c1]


def beyond_ln_table():
    """[(name, Case)].  Coverages this large leave a likelihood above exp(-745) only where the counts sit at the mode of the
    genotype's multinomial, so each family picks the rate that puts two genotypes there at once:
      thirds   diploid, three alleles, rate float(1/3): a heterozygote's (1-e)/2, (1-e)/2, e are 1/3 each, the three of them are
               one multinomial and differ by their priors and by the ln arguments n, c_i + c_j they take
      skewed   diploid, three alleles, rate 0.3, coverages about (0.35, 0.325 + d, 0.325 - d) n: 0/1 and 0/2 compete, the priors
               make up for (0.35 / 0.3)^(2 d)
      halves   haploid, two alleles, rate 0.5 (a haploid record with more alleles loses (A-1)^-errors and with another rate
               (1-e / e)^(c0 - c1)): the two genotypes take ln(c0) and ln(c1) in opposite order
    Totals straddle 65535 / 65536 / 65537 and go up to 10^6; records whose total is at most 65535 take every ln from the table."""
    rng = np.random.default_rng(2024)
    totals = [65535, 65535, 65536, 65537, 65538, 98304, 99999, 100000, 131071, 131072, 196608, 262144, 300000, 524288, 999999, 1000000]
    lows = [30000, 50000, 60000, 65000, 65534, 65535]
    thirds = [([32767, 32768, 32769], rng.dirichlet(np.ones(3) * 50)),       # pair sums 65535, 65536, 65537
              ([21845, 21845, 21845], rng.dirichlet(np.ones(3) * 50)),       # total 65535: all from the table
              ([21845, 21845, 21846], rng.dirichlet(np.ones(3) * 50))]       # total 65536: ln(n) alone leaves it
    for n in (totals + lows) * 4:
        thirds.append((_thirds(rng, n), rng.dirichlet(np.ones(3) * 50)))
    skewed = [([40000, 30000, 30000], [0.4, 0.3, 0.3]), ([40000, 30004, 29996], [0.4, 0.1, 0.1 * np.exp(8 * 0.15415)])]
    for n in (totals[:-3] + lows) * 3:                                     # at 5e5 and beyond the second heterozygote is 0
        d = int(rng.integers(-25, 26))
        c0 = int(round(0.35 * n)) + int(rng.integers(-40, 41))
        c1 = (n - c0) // 2 + d
        c2 = n - c0 - c1
        f1 = float(rng.uniform(0.001, 0.01))
        f2 = f1 * np.exp((c1 - c2) * 0.15415 + rng.uniform(-2, 2))          # ln(0.35 / 0.3) = 0.15415
        skewed.append(([c0, c1, c2], [0.5, f1, f2]))
    halves = [([32767, 32768], [0.5, 0.5]), ([32766, 32770], [0.4, 0.6]), ([32768, 32769], [0.5, 0.5])]
    for n in (totals + lows) * 4:
        c0 = n // 2 + int(np.rint(rng.normal(0, 0.5 * np.sqrt(n))))
        halves.append(([c0, n - c0], rng.dirichlet(np.ones(2) * 20)))
    return [("thirds", pack(thirds, THIRD, BIG_MAX_COV, False)), ("skewed", pack(skewed, 0.3, BIG_MAX_COV, False)),
            ("halves", pack(halves, 0.5, BIG_MAX_COV, True))]


def beyond_ln_sample():
    """[(name, Case)]: 3000 `thirds` and 1500 `halves` records at random totals of 65,536 .. 10^6 (uniform in ln n).  The
    device's log(double) is a last bit away from libm's for about one such record in 250: a sample this
    large holds a dozen of them, the handful of `beyond_ln_table` happens to hold none."""
    rng = np.random.default_rng(77)

    def totals(k):
        return [int(n) for n in np.exp(rng.uniform(np.log(LN_TABLE), np.log(10 ** 6), size=k)).astype(np.int64).clip(LN_TABLE, 10 ** 6)]
    thirds = [(_thirds(rng, n), rng.dirichlet(np.ones(3) * 50)) for n in totals(3000)]
    halves = []
    for n in totals(1500):
        c0 = n // 2 + int(np.rint(rng.normal(0, 0.5 * np.sqrt(n))))
        halves.append(([c0, n - c0], rng.dirichlet(np.ones(2) * 20)))
    return [("thirds", pack(thirds, THIRD, BIG_MAX_COV, False)), ("halves", pack(halves, 0.5, BIG_MAX_COV, True))]


def beyond_table(case):
    """per record: does a genotype take ln(n) of an n >= 65536?  The total is the largest argument there is."""
    return np.array([int(np.asarray(c, np.int64).sum()) >= LN_TABLE for c, _ in records(case)])


# ---- D: the branches of logf --------------------------------------------------------------------------------------------
def logf_interval(x):
    """table interval logf picks for a positive normal float: bits 19..22 of ix - 0x3f330000"""
    ix = int(np.float32(x).view(np.uint32))
    return ((ix - 0x3f330000) & 0xffffffff) >> 19 & 15


def logf_branch(x):
    x = np.float32(x)
    ix = int(x.view(np.uint32))
    if ix == 0x3f800000:
        return "one"
    if ix * 2 & 0xffffffff == 0:
        return "zero"
    if ix == 0x7f800000:
        return "inf"
    if ix & 0x80000000 or (ix * 2 & 0xffffffff) >= 0xff000000:
        return "nan"                                   # negative or NaN
    if ix < 0x00800000:
        return "subnormal"
    return "min_normal" if ix == 0x00800000 else "above_one" if ix > 0x3f800000 else "normal"


def logf_args(case):
    """per record, the floats logf is called with for the priors: freq[g] (haploid, homozygous), 2 * f1 * f2 (heterozygous)"""
    out = []
    two = np.float32(2)
    with np.errstate(all="ignore"):
        for _, f in records(case):
            args = [("freq", x) for x in f]
            if not case.haploid:
                args += [("pair", two * f[i] * f[j]) for i in range(len(f)) for j in range(i + 1, len(f))]
            out.append(args)
    return out


LOGF_BRANCHES_FREQ = ("subnormal", "min_normal", "one", "above_one", "nan", "inf", "zero")
LOGF_BRANCHES_PAIR = ("subnormal", "zero")
_SPECIAL = (1e-40, 1e-45, float(F32_MIN_NORMAL), 1.0, 1.5, -0.5, float("nan"), float("inf"))
_PAIRS = ((1e-20, 1e-20), (3e-20, 2e-21), (1e-19, 5e-22), (1e-15, 4e-25),      # 2 f1 f2 subnormal
          (1e-30, 1e-30), (1e-25, 1e-22), (1e-38, 1e-10), (2e-23, 1e-23))      # 2 f1 f2 underflows to 0


def logf_specials(haploid, seed=5):
    """every special frequency, and (diploid) every pair with a subnormal or vanishing product, in two- and three-allele
    records at ordinary coverage: the special value at each allele position in turn, four coverage draws each"""
    rng = np.random.default_rng(seed)
    recs = []
    for rep in range(4):
        for A in (2, 3):
            for x in _SPECIAL:
                for at in range(A):
                    f = rng.dirichlet(np.ones(A))
                    f[at] = x
                    recs.append((rng.integers(1, 30, size=A), f))
            for f1, f2 in _PAIRS:
                f = rng.dirichlet(np.ones(A))
                f[0], f[A - 1] = f1, f2
                recs.append((rng.integers(1, 30, size=A), f))
    return pack(recs, 0.001, 200, haploid)


def logf_sweep(haploid):
    """16 x 8 biallelic records (0.5, f): 2 * 0.5 * f = f exactly, f in each of logf's 16 table intervals at eight exponents"""
    rng = np.random.default_rng(16)
    recs = []
    for i in range(16):
        for j in range(8):
            bits = 0x3f330000 + (i << 19) + int(rng.integers(0, 1 << 19))
            f = float(np.uint32(bits).view(np.float32)) * 2.0 ** -(3 * j)
            recs.append((rng.integers(1, 12, size=2), [0.5, f]))
    return pack(recs, 0.001, 200, haploid)


# ---- E: error rates and max_cov ------------------------------------------------------------------------------------------
RATES = (0.0, 1e-8, 0.01, 0.5, 1.0)
MAX_COVS = (0, 1, 59, 60)


def mixed(error_rate, haploid, max_cov=200, n=500, seed=9, amax=6):
    """the shapes of the random test (2..6 alleles, uncovered / over-covered / partly covered records, a zero frequency); the
    records do not depend on the rate or on max_cov"""
    rng = np.random.default_rng(seed)
    recs = []
    for v in range(n):
        a = int(rng.integers(2, amax + 1))
        mode = rng.integers(0, 10)
        c = rng.integers(0, 60, size=a)
        if mode == 0:
            c[:] = 0
        elif mode == 1:
            c[rng.integers(0, a)] = 201 + rng.integers(0, 100)
        elif mode >= 6:
            c[rng.integers(0, a):] = 0
        f = rng.dirichlet(np.ones(a))
        if mode == 3:
            f[rng.integers(0, a)] = 0
        recs.append((c, f))
    return pack(recs, error_rate, max_cov, haploid)


def at_max_cov(max_cov, haploid, n=400, seed=13):
    """coverages 0..60 against a small max_cov; every fourth record has its largest coverage at max_cov, every fourth (from
    1) at max_cov + 1"""
    rng = np.random.default_rng(seed + max_cov)
    recs = []
    for v in range(n):
        a = int(rng.integers(2, 5))
        c = rng.integers(0, 61, size=a)
        if v % 4 < 2:
            c = np.minimum(c, max_cov)
            c[rng.integers(0, a)] = max_cov + v % 4
        recs.append((c, rng.dirichlet(np.ones(a))))
    return pack(recs, 0.001, max_cov, haploid)


# ---- F: every raw value subnormal or zero ---------------------------------------------------------------------------------
def tiny(haploid):
    """Haploid: three alleles at 1/3 and coverages around (54, 54, 54), whose three values are 1.965e-313.  Diploid: three
    alleles and coverages around (145, 145, 145), where the heterozygotes' error term (cov of the third allele times ln 0.001)
    brings them to exp(-725) and the homozygotes are 0."""
    lo, hi = (49, 60) if haploid else (139, 151)
    recs = [([a, b, c], [THIRD] * 3) for a in range(lo, hi) for b in range(lo, hi) for c in range(lo, hi)]
    return pack(recs, 0.001, 200, haploid)


def all_tiny(exp):
    """per record: status normal, no raw value at or above the smallest normal double, at least one above 0"""
    out = np.zeros(len(exp.status), dtype=bool)
    for v in range(len(out)):
        r = exp.raw[int(exp.goff[v]):int(exp.goff[v + 1])]
        out[v] = exp.status[v] == ST_NORMAL and bool(np.all(r < 2.2250738585072014e-308) and np.any(r > 0))
    return out
