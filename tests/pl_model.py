"""The definition of mg_phred_likelihoods (include/malva_hip.h) restated in Python: the likelihood part of the genotyper -- log_post of
gt_value, csrc/geno_dev.h -- scaled to Phred and rounded.  A helper, not a test: tests/test_pl_cpu.py pins it against the oracle's raw
genotype values (which makes it an authority), tests/test_gpu_pl.py holds the device against it, bit for bit.

logf is the host libm's (ctypes: numpy's float32 log is not glibc's), ln(n) is math.log(float(n)), the (float)count * constant products
are numpy.float32 products, everything else is Python floats (doubles), each operation rounded on its own."""
import ctypes
import ctypes.util
import functools
import math

import numpy as np

MISSING = -2 ** 31                                   # MG_PL_MISSING
K = float.fromhex("0x1.15f2ced384f29p+2")            # the double nearest to 10 / ln 10 (10 / math.log(10) is one ulp below it)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
F = np.float32


def logf(x):
    """glibc's logf of a float32 -> float32"""
    return F(_libm.logf(ctypes.c_float(float(x))))


def ln(n):
    return math.log(float(n))


def log_binomial(n, k):
    if n == 0 or n == k or k == 0:
        return 0.0
    return n * ln(n) - k * ln(k) - (n - k) * ln(n - k)


@functools.lru_cache(maxsize=None)
def constants(error_rate, A):
    """-> (c_hom, c_het, c_err1, c_err2) as float32, the way fill_geno_params and the oracle make them"""
    e = F(error_rate)
    with np.errstate(all="ignore"):
        return (logf(F(1) - e), logf((F(1) - e) / F(2)), logf(e / F(A - 1)) if A > 1 else None, logf(e / F(A - 2)) if A > 2 else None)


def log_post(cov, g1, g2, error_rate):
    """log of the likelihood of genotype (g1, g2) of a cell with the coverages cov; g2 < 0 or g1 == g2: the homozygous / haploid form"""
    A = len(cov)
    total = sum(cov)
    c_hom, c_het, c_err1, c_err2 = constants(float(F(error_rate)), A)
    with np.errstate(all="ignore"):
        if g2 < 0 or g1 == g2:
            truth = cov[g1]
            error = total - truth
            return log_binomial(truth + error, truth) + float(F(truth) * c_hom) + float(F(error) * c_err1)
        t1, t2 = cov[g1], cov[g2]
        error = total - t1 - t2
        lp = log_binomial(t1 + t2 + error, t1 + t2) + log_binomial(t1 + t2, t1) + float(F(t1) * c_het) + float(F(t2) * c_het)
        if A > 2:
            lp += float(F(error) * c_err2)
        return lp


def log_prior(freq, g1, g2):
    """the prior gt_value folds in (for the pin against the oracle); freq: float32 values"""
    with np.errstate(all="ignore"):
        if g2 < 0 or g1 == g2:
            return float(F(2) * logf(F(freq[g1])))
        return float(logf(F(2) * F(freq[g1]) * F(freq[g2])))


def genotypes(A, haploid):
    """the genotypes of a record in VCF order: j/k (j <= k) at index k (k + 1) / 2 + j; haploid: the allele"""
    if haploid:
        return [(a, -1) for a in range(A)]
    return [(j, k) for k in range(A) for j in range(k + 1)]


@functools.lru_cache(maxsize=None)
def cell_lps(cov, error_rate, max_cov, haploid):
    """cov: tuple of ints -> "over", "single", or the list of lp_g in VCF order (steps 1, 2 and 4 of the definition)"""
    A = len(cov)
    if any(c > max_cov for c in cov):
        return "over"
    if A == 1:
        return "single"
    return [log_post(cov, g1, g2, error_rate) for g1, g2 in genotypes(A, haploid)]


def scale(lps, cap):
    """steps 5 and 6"""
    finite = [x for x in lps if math.isfinite(x)]
    if not finite:
        return [MISSING] * len(lps)
    M = max(finite)
    out = []
    for lp in lps:
        if math.isnan(lp) or lp == math.inf:
            out.append(MISSING)
            continue
        d = M - lp
        x = d * K
        out.append(cap if x >= float(cap) else int(x + 0.5))
    return out


def pl_cell(cov, error_rate, max_cov, haploid, cap):
    """one cell -> its G values in VCF order (A == 0: none)"""
    cov = tuple(int(c) for c in cov)
    A = len(cov)
    if A == 0:
        return []
    lps = cell_lps(cov, float(F(error_rate)), int(max_cov), bool(haploid))
    if lps == "over":
        return [MISSING] * (A if haploid else A * (A + 1) // 2)
    if lps == "single":
        return [0]
    return scale(lps, cap)


def gt_offsets(var_allele_off, haploid):
    A = np.diff(np.asarray(var_allele_off, dtype=np.int64))
    off = np.zeros(len(A) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(A if haploid else A * (A + 1) // 2)
    return off


def pl_array(cov, var_allele_off, error_rate, max_cov, haploid, cap):
    """cov: [planes, slots] -> (pl [planes, var_gt_off[-1]] int32, var_gt_off)"""
    cov = np.asarray(cov)
    vao = [int(x) for x in var_allele_off]
    vgo = gt_offsets(var_allele_off, haploid)
    out = np.zeros((cov.shape[0], int(vgo[-1])), dtype=np.int32)
    for p in range(cov.shape[0]):
        row = cov[p].tolist()
        for v in range(len(vao) - 1):
            out[p, int(vgo[v]):int(vgo[v + 1])] = pl_cell(row[vao[v]:vao[v + 1]], error_rate, max_cov, haploid, cap)
    return out, vgo
