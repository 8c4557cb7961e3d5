"""The definition of mg_genotype_cohort (include/malva_hip.h) in numpy: allele priors re-estimated from the planes of a batch, then
every cell genotyped under them.  A helper, not a test: tests/test_cohort_priors_cpu.py pins it on hand-computed cases,
tests/test_gpu_cohort_priors.py holds the device against it bit for bit.

A plane's raw genotype values come from the oracle (oracle.capi.genotype: VB::genotype restated in C with the host's libm), the
normalised list, GT and GQ from oracle.capi.select_gt.  What this file adds is the part the reference does not have: the status
from the coverages, the expected allele copies, the sum over planes in its fixed tree order (an explicit loop over
x[i] + x[i + s] in float64) and the update with its float32 casts.  Python floats are IEEE doubles, every operation rounded on
its own."""
import numpy as np

from oracle import capi as ocapi

MAX_ALLELES = 8                                    # MG_PRIOR_MAX_ALLELES
NORMAL, OVERCOV, SINGLE, NOCOV = 0, 1, 2, 3        # MG_GT_*


def cell_status(cov, max_cov):
    """the status genotype_one gives a cell: from the coverages alone"""
    c = np.asarray(cov, dtype=np.uint32).view(np.int32).astype(np.int64)        # (int)cov[a]
    if (c > max_cov).any():
        return OVERCOV
    if len(c) == 1:
        return SINGLE
    if int(c.sum()) % (1 << 32) == 0:
        return NOCOV
    return NORMAL


def raw_values(cov, f, error_rate, max_cov, haploid):
    """-> [(g1, g2, value)] in the reference's list order, for a cell whose status is NORMAL"""
    return ocapi.genotype(cov, f, error_rate, max_cov, haploid)


def expected_copies(cov, f, error_rate, max_cov, haploid):
    """one plane in one iteration -> (counts, e[A]): e[a] walks the genotype list in order"""
    A = len(cov)
    lst = raw_values(cov, f, error_rate, max_cov, haploid)
    total = 0.0
    for _, _, val in lst:
        total = total + val
    if not (np.isfinite(total) and total > 0):
        return False, [0.0] * A
    e = []
    for a in range(A):
        x = 0.0
        for g1, g2, val in lst:
            q = val / total
            if haploid:
                if g1 == a:
                    x = x + q
            elif g1 == a and g2 == a:
                x = x + 2.0 * q
            elif g1 == a or g2 == a:
                x = x + q
        e.append(x)
    return True, e


def tree_sum(values, n_planes):
    """x[i] = values[i] below n_planes, +0.0 above, up to the next power of two; s = P'/2 .. 1: x[i] = x[i] + x[i + s], i < s"""
    pp = 1
    while pp < n_planes:
        pp *= 2
    x = [float(values[i]) if i < n_planes else 0.0 for i in range(pp)]
    s = pp // 2
    while s >= 1:
        for i in range(s):
            x[i] = x[i] + x[i + s]
        s //= 2
    return x[0]


def update(c, n, f0, ploidy, weight):
    """-> f_t (float32 [A]) from the summed copies c[A] (c[0] is not read), n > 0 planes that count and the panel's f0"""
    A = len(f0)
    new = np.zeros(A, dtype=np.float32)
    for a in range(1, A):
        wf = float(weight) * float(f0[a])
        num = float(c[a]) + wf
        den = float(ploidy * n) + float(weight)
        with np.errstate(all="ignore"):
            new[a] = np.float32(np.float64(num) / np.float64(den))
    acc = 0.0
    acc = acc + float(np.float32(0.0))
    for a in range(1, A):
        acc = acc + float(new[a])
    with np.errstate(all="ignore"):
        r = np.float32(1.0 - acc)
    new[0] = np.float32(0.0) if r < 0 else r
    return new


def estimate_record(cov, f0, error_rate, max_cov, haploid, iters, weight, early_stop=True):
    """cov: [P, A] uint32, f0: [A] float32 -> (f_T float32 [A], n of the last iteration that ran)"""
    cov = np.asarray(cov, dtype=np.uint32)
    f0 = np.asarray(f0, dtype=np.float32)
    P, A = cov.shape
    if not (2 <= A <= MAX_ALLELES and iters > 0):
        return f0.copy(), 0
    normal = [cell_status(cov[p], max_cov) == NORMAL for p in range(P)]
    f, n = f0.copy(), 0
    for _ in range(iters):
        e, n = np.zeros((P, A), dtype=np.float64), 0
        for p in range(P):
            if normal[p]:
                counts, ep = expected_copies(cov[p], f, error_rate, max_cov, haploid)
                if counts:
                    n += 1
                    e[p] = ep
        if n == 0:
            if early_stop:
                break
            continue                                                                # the frequencies stay as they are
        c = [tree_sum(e[:, a], P) for a in range(A)]
        new = update(c, n, f0, 1 if haploid else 2, weight)
        same = new.view(np.uint32).tolist() == f.view(np.uint32).tolist()
        f = new
        if same and early_stop:
            break
    return f, n


def genotype_cell(cov, f, error_rate, max_cov, haploid):
    """-> (gt1, gt2, gq, status, normalised list or None): genotype_one"""
    st = cell_status(cov, max_cov)
    d2 = -1 if haploid else 0
    if st != NORMAL:
        return 0, d2, 100 if st == SINGLE else 0, st, None
    lst = raw_values(cov, f, error_rate, max_cov, haploid)
    with np.errstate(all="ignore"):
        bi, gq, norm = ocapi.select_gt([x[2] for x in lst])
    if bi < 0:
        return 0, d2, gq, st, norm
    return lst[bi][0], lst[bi][1], gq, st, norm


def gt_offsets(var_allele_off, haploid):
    A = np.diff(np.asarray(var_allele_off, dtype=np.int64))
    goff = np.zeros(len(A) + 1, dtype=np.uint64)
    goff[1:] = np.cumsum(A if haploid else A * (A + 1) // 2)
    return goff


def genotype_cohort(cov, freq, var_allele_off, error_rate, max_cov, haploid, iters, weight, early_stop=True):
    """the whole entry -> (freq_out, n_informative, gt1, gt2, gq, status, probs [P, G], var_gt_off); probs of a cell whose status is not
    NORMAL are left at 0"""
    cov = np.asarray(cov, dtype=np.uint32)
    freq = np.asarray(freq, dtype=np.float32)
    vo = np.asarray(var_allele_off, dtype=np.int64)
    P, n = cov.shape[0], len(vo) - 1
    goff = gt_offsets(vo, haploid)
    fo, ni = freq.copy(), np.zeros(n, dtype=np.uint32)
    g1, g2, gq = (np.zeros((P, n), dtype=np.int32) for _ in range(3))
    st = np.zeros((P, n), dtype=np.uint8)
    probs = np.zeros((P, int(goff[-1])), dtype=np.float64)
    for v in range(n):
        a0, a1 = int(vo[v]), int(vo[v + 1])
        fo[a0:a1], ni[v] = estimate_record(cov[:, a0:a1], freq[a0:a1], error_rate, max_cov, haploid, iters, weight, early_stop)
        for p in range(P):
            g1[p, v], g2[p, v], gq[p, v], st[p, v], norm = genotype_cell(cov[p, a0:a1], fo[a0:a1], error_rate, max_cov, haploid)
            if norm is not None:
                probs[p, int(goff[v]):int(goff[v + 1])] = norm
    return fo, ni, g1, g2, gq, st, probs, goff


# ---- inputs for the tests ---------------------------------------------------------------------------------------------------------

ALLELE_COUNTS = (2, 3, 2, 1, 4, 2, 8, 9, 2, 2, 3, 2)   # record v has ALLELE_COUNTS[v % 12] alleles: the first four records already mix 1, 2 and 3


def synth_batch(seed, n_planes, n_vars, haploid, max_cov=200):
    """a cohort whose allele frequencies are NOT the panel's -> (cov [P, slots] uint32, freq [slots] float32, var_allele_off): per record
    a panel AF per ALT allele between 1e-4 and 0.2 (REF by the parser's rule), an unrelated cohort frequency, and per plane a genotype
    drawn from the cohort's with reads at a depth of 1..40 (three times in ten: 1 or 2) split over its alleles and a stray read now and then; about one cell in
    seven is instead without coverage, over-covered (max_cov + 1 .. max_cov + 20) or noise in 0..max_cov"""
    rng = np.random.default_rng(seed)
    A = np.array([ALLELE_COUNTS[v % len(ALLELE_COUNTS)] for v in range(n_vars)], dtype=np.int64)
    vo = np.zeros(n_vars + 1, dtype=np.uint32)
    vo[1:] = np.cumsum(A)
    slots = int(vo[-1])
    freq = np.zeros(slots, dtype=np.float32)
    cov = np.zeros((n_planes, slots), dtype=np.uint32)
    for v in range(n_vars):
        a0, n_all = int(vo[v]), int(A[v])
        alt = (10.0 ** rng.uniform(-4.0, -0.7, n_all - 1)).astype(np.float32)
        acc = 0.0
        for x in alt:
            acc += float(x)
        freq[a0] = max(np.float32(1.0 - acc), np.float32(0.0))
        freq[a0 + 1:a0 + n_all] = alt
        truth = rng.dirichlet(np.full(n_all, 0.7))
        for p in range(n_planes):
            kind = rng.random()
            row = np.zeros(n_all, dtype=np.int64)
            if kind < 0.05:
                pass
            elif kind < 0.10:
                row[:] = rng.integers(0, 30, n_all)
                row[rng.integers(0, n_all)] = max_cov + rng.integers(1, 21)
            elif kind < 0.15:
                row[:] = rng.integers(0, max_cov + 1, n_all)
            else:
                depth = int(rng.integers(1, 3)) if rng.random() < 0.3 else int(rng.integers(1, 41))   # (a read or two: the prior decides)
                copies = rng.choice(n_all, size=1 if haploid else 2, p=truth)
                for r in rng.choice(copies, size=depth):
                    row[r] += 1
                if rng.random() < 0.2:
                    row[rng.integers(0, n_all)] += 1
            cov[p, a0:a0 + n_all] = row
    return cov, freq, vo
