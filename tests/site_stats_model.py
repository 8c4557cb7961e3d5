"""The per-record table of `call --cohort --site-stats` restated: the genotype counts of mg_site_geno_counts in numpy, the exact test
of mg_hwe_exact in plain Python floats -- every step one IEEE double operation, in the order include/malva_hip.h fixes, so that the
device's results can be compared bit for bit -- and the table's text."""
import math

import numpy as np

HEADER = "#CHROM\tPOS\tID\tREF\tALT\tSAMPLES\tN\tAN\tAC\tAF\tHOM\tHET\tHWE\tEXC_HET\n"
HWE_MAX_N = 1 << 24                                                                # MG_HWE_MAX_N
NAN = float("nan")


def geno_counts_plain(gt1, gt2, gq, haploid, var_allele_off, min_gq=None):
    """gt1 / gt2 / gq: [planes, n_vars] -> (n [n_vars], het [slots], hom [slots]) uint32.  A cell is usable when it is not masked
    (gq < min_gq) and every index the mode reads lies in [0, A)."""
    g1 = np.asarray(gt1, dtype=np.int64)
    g2 = g1 if haploid else np.asarray(gt2, dtype=np.int64)
    vao = np.asarray(var_allele_off, dtype=np.int64)
    planes, nv = g1.shape
    A = np.diff(vao)[None, :]
    usable = (g1 >= 0) & (g1 < A) & (g2 >= 0) & (g2 < A)
    if min_gq is not None:
        usable &= np.asarray(gq, dtype=np.int64) >= min_gq
    slots = int(vao[nv]) if nv else 0
    het, hom = np.zeros(slots, dtype=np.int64), np.zeros(slots, dtype=np.int64)
    base = np.broadcast_to(vao[None, :-1], g1.shape)
    same = usable & (g1 == g2)
    diff = usable & (g1 != g2)
    np.add.at(hom, (base + g1)[same], 1)
    np.add.at(het, (base + g1)[diff], 1)
    np.add.at(het, (base + g2)[diff], 1)
    return usable.sum(axis=0).astype(np.uint32), het.astype(np.uint32), hom.astype(np.uint32)


def hwe_exact(n, het, hom):
    """-> (hwe, exc_het): mg_hwe_exact's definition, operation by operation"""
    n, het, hom = int(n), int(het), int(hom)
    if het + hom > n or n > HWE_MAX_N:
        return NAN, NAN
    na = het + 2 * hom
    nb = 2 * n - na
    r = min(na, nb)
    mid = r * (2 * n - r) // (2 * n) if n else 0
    if (mid ^ r) & 1:
        mid += 1
    hr0 = (r - mid) // 2
    hc0 = n - mid - hr0

    def down(q, h, hr, hc):
        return q * (float(h * (h - 1)) / float(4 * (hr + 1) * (hc + 1)))

    def up(q, h, hr, hc):
        return q * (float(4 * hr * hc) / float((h + 2) * (h + 1)))

    q_obs, h, hr, hc = 1.0, mid, hr0, hc0
    while h > het:
        q_obs = down(q_obs, h, hr, hc)
        h, hr, hc = h - 2, hr + 1, hc + 1
    while h < het:
        q_obs = up(q_obs, h, hr, hc)
        h, hr, hc = h + 2, hr - 1, hc - 1
    S = 1.0
    L = 1.0 if 1.0 <= q_obs else 0.0
    G = 1.0 if mid >= het else 0.0
    q, h, hr, hc = 1.0, mid, hr0, hc0
    while h > 1:
        q = down(q, h, hr, hc)
        h, hr, hc = h - 2, hr + 1, hc + 1
        S += q
        if q <= q_obs:
            L += q
        if h >= het:
            G += q
    q, h, hr, hc = 1.0, mid, hr0, hc0
    while h + 2 <= r:
        q = up(q, h, hr, hc)
        h, hr, hc = h + 2, hr - 1, hc - 1
        S += q
        if q <= q_obs:
            L += q
        if h >= het:
            G += q
    return min(L / S, 1.0), min(G / S, 1.0)


def af_text(ac, an):
    """mg_format_site_info's integer rule: six decimals rounded half up, trailing zeros dropped, `0`, `1`, `.` when AN = 0"""
    if an == 0:
        return "."
    q = (2 * ac * 1000000 + an) // (2 * an)
    if q == 0 or q >= 1000000:
        return "1" if q else "0"
    return "0." + ("%06d" % q).rstrip("0")


def site_stats_text(cols, samples, haploid, var_allele_off, n, het, hom, hwe=hwe_exact):
    """cols: per record its first five columns joined by tabs -> the table's text.  hwe: the test, (n, het, hom) -> (p, p)."""
    out = [HEADER]
    for v, c in enumerate(cols):
        a0, a1 = int(var_allele_off[v]), int(var_allele_off[v + 1])
        if a1 - a0 < 2:
            continue
        N = int(n[v])
        an = N if haploid else 2 * N
        alts = range(a0 + 1, a1)
        ac = [int(hom[s]) if haploid else int(het[s]) + 2 * int(hom[s]) for s in alts]
        if haploid or N == 0:
            p = e = ["."] * len(ac)
        else:
            tests = [hwe(N, int(het[s]), int(hom[s])) for s in alts]
            p, e = ["%.6g" % t[0] for t in tests], ["%.6g" % t[1] for t in tests]
        lists = [[str(x) for x in ac], [af_text(x, an) for x in ac], [str(int(hom[s])) for s in alts], [str(int(het[s])) for s in alts], p, e]
        out.append("\t".join([c, str(samples), str(N), str(an)] + [",".join(l) for l in lists]) + "\n")
    return "".join(out)


def is_nan(x):
    return isinstance(x, float) and math.isnan(x)
