"""A plain restatement of the genetic relationship matrix (`call --cohort --grm`, mg_grm_weights / mg_grm_begin / mg_grm_step in
include/malva_hip.h): the records' weights in 16-bit fixed point, the pairs' sums, and the table's text from a parsed merged VCF.  The
weights use numpy's binary64 sqrt, divide and rint -- IEEE operations, as the definition names them -- and everything else is an integer,
so the device, the host and this file agree exactly."""
import numpy as np

from ibd_model import dosage_from_words
from ld_model import parse_merged_vcf, site_words

SHIFT, MAX_Q, MAX_SAMPLES = 10, 32639, 16384
HEADER = "#A\tB\tN\tGRM\n"


def weights_from_counts(n0, n1, n2, haploid=False, maf_ppm=0, min_n=1):
    """the records' counts of dosage 0, 1, 2 -> (q int64 [..., 3], enters bool [...]); q is what the formula gives wherever D > 0 (0
    elsewhere), whether the record enters or not"""
    n0, n1, n2 = (np.asarray(x, dtype=np.int64) for x in (n0, n1, n2))
    if haploid:
        n = n0 + n2
        an, ac = n, n2
        D = 4 * ac * (an - ac)
    else:
        n = n0 + n1 + n2
        an, ac = 2 * n, n1 + 2 * n2
        D = 2 * ac * (an - ac)
    assert (D < 2 ** 31).all()
    root = np.sqrt(np.where(D > 0, D, 1).astype(np.float64))
    q = np.stack([np.rint(((d * an - 2 * ac) * (1 << SHIFT)).astype(np.float64) / root).astype(np.int64) for d in range(3)], axis=-1)
    q[D <= 0] = 0
    enters = (D > 0) & (n >= min_n) & (np.minimum(ac, an - ac) * 1000000 >= maf_ppm * an) & (np.abs(q) <= MAX_Q).all(axis=-1)
    return q, enters


def counts_from_dosage(D):
    """int [n_vars, n_samples], -1 where the cell does not contribute -> n0, n1, n2 per record"""
    D = np.asarray(D, dtype=np.int64)
    return tuple((D == d).sum(axis=1) for d in range(3))


def weights_table(D, haploid=False, maf_ppm=0, min_n=1):
    """what mg_grm_weights returns: int16 [n_vars, 4], q0 q1 q2 1 of a record that enters, zeros of one that does not"""
    D = np.asarray(D, dtype=np.int64)
    if haploid:
        D = np.where(D == 1, -1, D)
    q, enters = weights_from_counts(*counts_from_dosage(D), haploid=haploid, maf_ppm=maf_ppm, min_n=min_n)
    out = np.zeros((D.shape[0], 4), dtype=np.int16)
    out[enters, :3] = q[enters]
    out[enters, 3] = 1
    return out


def digits(q):
    """q -> (h, l), the balanced base-256 digits: q == 256 h + l, l in [-128, 127]"""
    q = np.asarray(q, dtype=np.int64)
    l = ((q + 128) & 255) - 128
    return (q - l) >> 8, l


def cell_weights(D, haploid=False, maf_ppm=0, min_n=1):
    """-> (X int64 [n_vars, n_samples], the weight of every cell, 0 where it does not count; C likewise, 1 where it counts; entered)"""
    D = np.asarray(D, dtype=np.int64)
    if haploid:
        D = np.where(D == 1, -1, D)
    w = weights_table(D, haploid, maf_ppm, min_n).astype(np.int64)
    counts = (D >= 0) & (w[:, 3:4] == 1)
    X = np.where(counts, np.take_along_axis(w[:, :3], np.clip(D, 0, 2), axis=1), 0)
    return X, counts.astype(np.int64), int(w[:, 3].sum())


def pair_index(n_samples):
    """the pairs a <= b, row-major, as two index vectors"""
    return np.triu_indices(n_samples)


def grm_sums(D, n_samples, haploid=False, maf_ppm=0, min_n=1):
    """-> (S int64 [n (n + 1) / 2], N uint64 likewise, records seen, records entered), as mg_grm_read gives them"""
    D = np.asarray(D, dtype=np.int64).reshape(-1, n_samples)
    X, Cc, entered = cell_weights(D, haploid, maf_ppm, min_n)
    assert np.abs(X).max(initial=0) ** 2 * max(D.shape[0], 1) < 2 ** 62
    a, b = pair_index(n_samples)
    S = (X.T @ X)[a, b]
    N = (Cc.T @ Cc)[a, b]
    return S.astype(np.int64), N.astype(np.uint64), D.shape[0], entered


def grm_sums_by_loop(D, n_samples, haploid=False, maf_ppm=0, min_n=1):
    """the same, the definition read out loud in Python integers: for small cases"""
    D = np.asarray(D, dtype=np.int64).reshape(-1, n_samples)
    w = weights_table(D, haploid, maf_ppm, min_n)
    S, N = [], []
    for a in range(n_samples):
        for b in range(a, n_samples):
            s = n = 0
            for v in range(D.shape[0]):
                da, db = int(D[v, a]), int(D[v, b])
                if haploid and 1 in (da, db):
                    continue
                if w[v, 3] and da >= 0 and db >= 0:
                    s += int(w[v, da]) * int(w[v, db])
                    n += 1
            S.append(s)
            N.append(n)
    return S, N, D.shape[0], int(w[:, 3].sum())


def words_from_dosage(D, n_samples, spare_bits=True):
    """int [n_vars, n_samples] -> uint64 [ceil(n_samples / 64), 3, n_vars], sample 64 g + p in bit p of group g; spare_bits: the bits at and
    beyond n_samples of the last group are SET in all three words (the library must mask them)"""
    D = np.asarray(D, dtype=np.int64).reshape(-1, n_samples)
    G = (n_samples + 63) // 64
    W = np.zeros((G, 3, D.shape[0]), dtype=np.uint64)
    for s in range(n_samples):
        g, p = divmod(s, 64)
        for d in range(3):
            W[g, d] |= (D[:, s] == d).astype(np.uint64) << np.uint64(p)
    if spare_bits and n_samples % 64:
        W[G - 1] |= np.uint64((1 << 64) - (1 << (n_samples % 64)))
    return W


def grm_text_value(s, n):
    """S 10^6 / (2^20 N) in six decimals, rounded half away from zero, from integers; `.` when N == 0"""
    s, n = int(s), int(n)
    if n == 0:
        return "."
    den = n << 20
    v = (2 * abs(s) * 10 ** 6 + den) // (2 * den)
    return "%s%d.%06d" % ("-" if s < 0 and v else "", v // 10 ** 6, v % 10 ** 6)


def parse_maf(text):
    """the decimal text of --grm-min-maf -> parts per million, exactly; None where the option refuses it"""
    head, dot, tail = text.partition(".")
    if not (head + tail).isdigit() or not head and not tail or len(tail) > 6 or len(head) > 1:
        return None
    ppm = int(head or "0") * 1000000 + int((tail + "000000")[:6])
    return ppm if ppm <= 500000 else None


def dosage_from_vcf(vcf_text, min_gq=None, group=64):
    """the merged VCF a run wrote -> (names, D int64 [n_vars, samples], haploid)"""
    names = next(l for l in vcf_text.split("\n") if l.startswith("#CHROM")).split("\t")[9:]
    cols, g1, g2, gq, vao, haploid = parse_merged_vcf(vcf_text)
    S = g1.shape[0]
    assert S == len(names)
    words = np.stack([site_words(g1[s:s + group], g2[s:s + group], gq[s:s + group], haploid, vao, min_gq) for s in range(0, S, group)])
    D = np.concatenate([dosage_from_words(words[g:g + 1], min(group, S - g * group)) for g in range(words.shape[0])], axis=1)
    return names, D, haploid


def grm_table_text(vcf_text, maf_ppm=10000, min_n=2, min_gq=None):
    """the bytes `--grm PATH` holds for the merged VCF a run wrote"""
    names, D, haploid = dosage_from_vcf(vcf_text, min_gq)
    S, N, _, _ = grm_sums(D, len(names), haploid, maf_ppm, min_n)
    a, b = pair_index(len(names))
    return HEADER + "".join("%s\t%s\t%d\t%s\n" % (names[i], names[j], int(n), grm_text_value(s, n)) for i, j, s, n in zip(a, b, S, N))


def gcta_values(S, N):
    """-> (float32 values, float32 counts) in GCTA's order: the lower triangle row by row, diagonal included.  Element (i, j), j <= i, is
    the pair a = j, b = i"""
    n = int(round((np.sqrt(8 * len(S) + 1) - 1) / 2))
    a, b = pair_index(n)
    full_s, full_n = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.uint64)
    full_s[b, a], full_n[b, a] = S, N
    i, j = np.tril_indices(n)
    s, k = full_s[i, j].astype(np.float64), full_n[i, j].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(k > 0, s / (k * 1048576.0), 0.0)
    return val.astype(np.float32), k.astype(np.float32)
