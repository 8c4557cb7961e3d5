"""The definition of mg_estimate_priors (include/malva_hip.h) in numpy: mg_genotype_cohort's estimate with the sum over planes
extended past 64.  A helper, not a test: tests/test_cohort_prior_wide_cpu.py pins it, tests/test_gpu_cohort_priors_wide.py holds the
device against it bit for bit.

Everything but the sum is tests/cohort_prior_model.py's: status, expected copies, the update.  The sum cuts the planes into chunks
of 64 in the order given, takes the model's fixed tree over each chunk (padded to the chunk's own power of two) and adds the
chunks' sums in order, each add rounded on its own."""
import numpy as np

import cohort_prior_model as M

CHUNK = 64
MAX_PLANES = 16384                                 # MG_PRIOR_WIDE_MAX_PLANES


def tree_sum(values, n_planes):
    """c = C_0, then c = c + C_j, j = 1, 2, ..; C_j = the model's tree over planes 64j .. min(64j + 64, P) - 1"""
    c = None
    for lo in range(0, n_planes, CHUNK):
        hi = min(lo + CHUNK, n_planes)
        cj = M.tree_sum(values[lo:hi], hi - lo)
        c = cj if c is None else c + cj
    return c


def estimate_record(cov, f0, error_rate, max_cov, haploid, iters, weight, early_stop=True):
    """cov: [P, A] uint32, f0: [A] float32 -> (f_T float32 [A], n of the last iteration that ran): M.estimate_record with the wide sum"""
    cov = np.asarray(cov, dtype=np.uint32)
    f0 = np.asarray(f0, dtype=np.float32)
    P, A = cov.shape
    if not (2 <= A <= M.MAX_ALLELES and iters > 0):
        return f0.copy(), 0
    normal = [M.cell_status(cov[p], max_cov) == M.NORMAL for p in range(P)]
    f, n = f0.copy(), 0
    for _ in range(iters):
        e, n = np.zeros((P, A), dtype=np.float64), 0
        for p in range(P):
            if normal[p]:
                counts, ep = M.expected_copies(cov[p], f, error_rate, max_cov, haploid)
                if counts:
                    n += 1
                    e[p] = ep
        if n == 0:
            if early_stop:
                break
            continue                                                                # the frequencies stay as they are
        c = [tree_sum(e[:, a], P) for a in range(A)]
        new = M.update(c, n, f0, 1 if haploid else 2, weight)
        same = new.view(np.uint32).tolist() == f.view(np.uint32).tolist()
        f = new
        if same and early_stop:
            break
    return f, n


def estimate_priors(cov, freq, var_allele_off, error_rate, max_cov, haploid, iters, weight, early_stop=True):
    """the whole entry -> (freq_out [slots] float32, n_informative [n_vars] uint32)"""
    cov = np.asarray(cov, dtype=np.uint32)
    freq = np.asarray(freq, dtype=np.float32)
    vo = np.asarray(var_allele_off, dtype=np.int64)
    n = len(vo) - 1
    fo, ni = freq.copy(), np.zeros(n, dtype=np.uint32)
    for v in range(n):
        a0, a1 = int(vo[v]), int(vo[v + 1])
        fo[a0:a1], ni[v] = estimate_record(cov[:, a0:a1], freq[a0:a1], error_rate, max_cov, haploid, iters, weight, early_stop)
    return fo, ni


def record_range(cov, freq, var_allele_off, lo, hi):
    """records [lo, hi) of a batch as a batch of their own -> (cov, freq, var_allele_off)"""
    vo = np.asarray(var_allele_off, dtype=np.int64)
    a0, a1 = int(vo[lo]), int(vo[hi])
    return np.ascontiguousarray(cov[:, a0:a1]), np.ascontiguousarray(freq[a0:a1]), (vo[lo:hi + 1] - a0).astype(np.uint32)
