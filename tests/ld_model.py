"""A plain numpy / Python-int restatement of the LD table (`call --cohort --ld`, mg_pack_site_dosage and mg_ld_window in
include/malva_hip.h): the words of a record over the samples, the pairs of a window with their r2, and the table's text from a parsed
merged VCF.  Everything is an integer up to one final division of two correctly rounded doubles, so the device, the host and this file
agree bit for bit."""
import numpy as np

LD_PAIR = np.dtype([("i", np.uint32), ("j", np.uint32), ("n", np.uint32), ("sign", np.int32), ("r2", np.float64)])
HEADER = "#CHROM\tPOS_A\tID_A\tPOS_B\tID_B\tN\tR2\tSIGN\n"
RULES = ("n_first", "window", "n_vars", "chrom", "max_bp", "min_n", "vx", "vy", "min_r2")


def site_words(g1, g2, gq, haploid, vao, min_gq):
    """gt1 / gt2 / gq [planes, n_vars] -> uint64 [3, n_vars]: bit p of [d, v] set when record v has two alleles, the cell (p, v) is called
    (min_gq None, or gq >= min_gq), every allele index the mode reads is 0 or 1 and the dosage -- gt1 + gt2, haploid 2 * gt1 -- is d"""
    g1 = np.asarray(g1, dtype=np.int64)
    g2 = g1 if haploid else np.asarray(g2, dtype=np.int64)
    planes, n = g1.shape
    ok = (np.diff(np.asarray(vao, dtype=np.int64)) == 2)[None, :] & (g1 >= 0) & (g1 <= 1) & (g2 >= 0) & (g2 <= 1)
    if min_gq is not None:
        ok = ok & (np.asarray(gq) >= min_gq)
    d = g1 + g2
    out = np.zeros((3, n), dtype=np.uint64)
    for p in range(planes):
        for dd in range(3):
            out[dd] |= np.where(ok[p] & (d[p] == dd), np.uint64(1) << np.uint64(p), np.uint64(0))
    return out


def words_from_dosage(D, group_sizes=None):
    """D [n_vars, samples], a dosage 0..2 or -1 (the cell does not contribute) -> uint64 [groups, 3, n_vars]; the samples fill groups of
    group_sizes (default: 64 each, the last one what is left)"""
    D = np.asarray(D, dtype=np.int64)
    n, S = D.shape
    if group_sizes is None:
        group_sizes = [min(64, S - s) for s in range(0, max(S, 1), 64)]
    assert sum(group_sizes) == S and all(1 <= g <= 64 for g in group_sizes)
    out = np.zeros((len(group_sizes), 3, n), dtype=np.uint64)
    s = 0
    for g, size in enumerate(group_sizes):
        for p in range(size):
            for d in range(3):
                out[g, d] |= np.where(D[:, s + p] == d, np.uint64(1) << np.uint64(p), np.uint64(0))
        s += size
    return out


def dosage_from_words(words):
    """uint64 [groups, 3, n_vars] -> (V, X) float64 [n_vars, samples in use]: V 1 where the cell contributes, X its dosage (0 elsewhere);
    bit columns no record uses are left out"""
    words = np.asarray(words, dtype=np.uint64)
    G, three, n = words.shape
    assert three == 3
    Vs, Xs = [], []
    for g in range(G):
        used = int(np.bitwise_or.reduce(words[g].reshape(-1))) if n else 0
        cols = np.array([p for p in range(64) if used >> p & 1], dtype=np.uint64)
        if not cols.size:
            continue
        b = [((words[g, d][:, None] >> cols[None, :]) & np.uint64(1)).astype(np.float64) for d in range(3)]
        assert not ((b[0] + b[1] + b[2]) > 1).any(), "a cell with two dosages"
        Vs.append(b[0] + b[1] + b[2])
        Xs.append(b[1] + 2 * b[2])
    if not Vs:
        return np.zeros((n, 0)), np.zeros((n, 0))
    return np.concatenate(Vs, axis=1), np.concatenate(Xs, axis=1)


def _sums(V, X, rows, cols):
    """the six sums of every pair (i in rows, j in cols) as int64 matrices (float64 products of small integers: exact)"""
    Vi, Xi, Vj, Xj = V[rows], X[rows], V[cols], X[cols]
    m = lambda a, b: np.rint(a @ b.T).astype(np.int64)
    return m(Vi, Vj), m(Xi, Vj), m(Vi, Xj), m(Xi * Xi, Vj), m(Vi, Xj * Xj), m(Xi, Xj)


def _r2(cov, vx, vy):
    """float(cov * cov) / float(vx * vy): each conversion rounds once to nearest even, then one IEEE division.  Products below 2^53 are
    doubles as they stand; the others are converted from Python ints"""
    num, den = cov * cov, vx * vy                 # (int64: at most 2^60)
    fn, fd = num.astype(np.float64), den.astype(np.float64)
    for src, dst in ((num, fn), (den, fd)):
        big = np.nonzero(src >= 1 << 53)[0]
        dst[big] = [float(x) for x in src[big].tolist()]
    return fn / fd


def ld_candidates(words, window, block=256):
    """every pair i < j <= i + window with vx > 0 and vy > 0, ordered by i, then j -> LD_PAIR array (what is left of the rules -- n_first,
    chrom, max_bp, min_n, min_r2 -- is ld_filter's)"""
    V, X = dosage_from_words(words)
    n = V.shape[0]
    assert window >= 1
    parts = []
    for i0 in range(0, n, block):
        i1, j0 = min(i0 + block, n), i0 + 1
        j1 = min(n, i1 + window)
        if j0 >= j1:
            continue
        rows, cols = np.arange(i0, i1), np.arange(j0, j1)
        N, Sx, Sy, Sxx, Syy, Sxy = _sums(V, X, rows, cols)
        I, J = rows[:, None], cols[None, :]
        cov, vx, vy = N * Sxy - Sx * Sy, N * Sxx - Sx * Sx, N * Syy - Sy * Sy
        ii, jj = np.nonzero((J > I) & (J <= I + window) & (vx > 0) & (vy > 0))                  # (row-major: by i, then j)
        out = np.zeros(ii.size, dtype=LD_PAIR)
        out["i"], out["j"], out["n"], out["sign"] = rows[ii], cols[jj], N[ii, jj], np.sign(cov[ii, jj])
        out["r2"] = _r2(cov[ii, jj], vx[ii, jj], vy[ii, jj])
        parts.append(out)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=LD_PAIR)


def ld_filter(cand, chrom, pos, n_first, max_bp, min_n, min_r2):
    """the candidates of ld_candidates that are emitted -> (pairs, row_off)"""
    chrom, pos = np.asarray(chrom, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    assert 0 <= n_first <= chrom.size and min_n >= 1 and 0.0 <= min_r2 <= 1.0
    i, j = cand["i"].astype(np.int64), cand["j"].astype(np.int64)
    keep = (i < n_first) & (chrom[i] == chrom[j]) & (cand["n"] >= min_n) & (cand["r2"] >= min_r2)
    if max_bp:
        keep &= np.abs(pos[j] - pos[i]) <= max_bp
    pairs = cand[keep]
    row_off = np.zeros(n_first + 1, dtype=np.uint64)
    row_off[1:] = np.cumsum(np.bincount(pairs["i"], minlength=n_first)[:n_first])
    return pairs, row_off


def ld_pairs(words, chrom, pos, n_first, window, max_bp, min_n, min_r2, block=256):
    """-> (pairs, row_off): the emitted pairs (LD_PAIR) ordered by i, then j, and uint64 [n_first + 1]"""
    return ld_filter(ld_candidates(words, window, block), chrom, pos, n_first, max_bp, min_n, min_r2)


def pair_sums(words, i, j):
    """-> (n, Sx, Sy, Sxx, Syy, Sxy) of one pair as Python ints, by popcounts of the words"""
    w = np.asarray(words, dtype=np.uint64)
    pc = lambda a: sum(bin(int(x)).count("1") for x in a)
    a0, a1, a2, b0, b1, b2 = w[:, 0, i], w[:, 1, i], w[:, 2, i], w[:, 0, j], w[:, 1, j], w[:, 2, j]
    A, B = a0 | a1 | a2, b0 | b1 | b2
    n, x1, x2, y1, y2 = pc(A & B), pc(a1 & B), pc(a2 & B), pc(A & b1), pc(A & b2)
    sxy = pc(a1 & b1) + 2 * (pc(a1 & b2) + pc(a2 & b1)) + 4 * pc(a2 & b2)
    return n, x1 + 2 * x2, y1 + 2 * y2, x1 + 4 * x2, y1 + 4 * y2, sxy


def pair_value(words, i, j):
    """-> (n, cov, vx, vy, r2 or None) of one pair, Python ints throughout"""
    n, sx, sy, sxx, syy, sxy = pair_sums(words, i, j)
    cov, vx, vy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    return n, cov, vx, vy, (float(cov * cov) / float(vx * vy) if vx > 0 and vy > 0 else None)


def why_not(words, chrom, pos, i, j, n_first, window, max_bp, min_n, min_r2):
    """the rules (of RULES) that keep the pair (i, j), i < j, out of the table; empty: it is emitted.  min_r2 is judged only where r2 exists."""
    n_vars = np.asarray(words).shape[2]
    out = set()
    if i >= n_first:
        out.add("n_first")
    if j > i + window:
        out.add("window")
    if j >= n_vars:
        return out | {"n_vars"}
    if chrom[i] != chrom[j]:
        out.add("chrom")
    if max_bp and abs(int(pos[j]) - int(pos[i])) > max_bp:
        out.add("max_bp")
    n, cov, vx, vy, r2 = pair_value(words, i, j)
    if n < min_n:
        out.add("min_n")
    if vx <= 0:
        out.add("vx")
    if vy <= 0:
        out.add("vy")
    if r2 is not None and r2 < min_r2:
        out.add("min_r2")
    return out


# ---- the table of the command line ------------------------------------------------------------------------------------------------

def parse_merged_vcf(text):
    """the merged VCF's text -> (cols, g1, g2, gq, vao, haploid): cols the records' first five columns, g1 / g2 / gq [samples, records]
    int32 (a missing allele -1, a missing GQ -1), vao the allele offsets"""
    cols, rows = [], []
    for line in text.split("\n"):
        if not line or line[0] == "#":
            continue
        f = line.split("\t")
        cols.append(f[:5])
        keys = f[8].split(":")
        gi, qi = keys.index("GT"), (keys.index("GQ") if "GQ" in keys else None)
        row = []
        for cell in f[9:]:
            parts = cell.split(":")
            gt = parts[gi].replace("|", "/").split("/")
            a = [-1 if x == "." else int(x) for x in gt]
            q = -1
            if qi is not None and qi < len(parts) and parts[qi] != ".":
                q = int(parts[qi])
            row.append((a[0], a[1] if len(a) > 1 else None, q))
        rows.append(row)
    n = len(rows)
    S = len(rows[0]) if n else 0
    haploid = n > 0 and all(c[1] is None for r in rows for c in r)
    g1, g2, gq = (np.zeros((S, n), dtype=np.int32) for _ in range(3))
    for v, r in enumerate(rows):
        for s, (a, b, q) in enumerate(r):
            g1[s, v], g2[s, v], gq[s, v] = a, (a if b is None else b), q
    A = [1 + (0 if c[4] == "." else len(c[4].split(","))) for c in cols]
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)
    return cols, g1, g2, gq, vao, haploid


def ld_table_text(vcf_text, window=64, max_bp=1000000, min_r2=0.2, min_n=2, min_gq=None, group=64):
    """the bytes `--ld PATH` holds for the merged VCF a run wrote: the samples in groups of `group` (the table does not depend on it)"""
    cols, g1, g2, gq, vao, haploid = parse_merged_vcf(vcf_text)
    n, S = len(cols), g1.shape[0]
    words = [site_words(g1[s:s + group], g2[s:s + group], gq[s:s + group], haploid, vao, min_gq) for s in range(0, S, group)]
    words = np.stack(words) if words else np.zeros((1, 3, n), dtype=np.uint64)
    chrom, last = np.zeros(n, dtype=np.uint32), None
    for v, c in enumerate(cols):                 # a running id that steps whenever the CHROM text changes
        chrom[v] = (chrom[v - 1] + (c[0] != last)) if v else 0
        last = c[0]
    pos = np.array([int(c[1]) for c in cols], dtype=np.uint32)
    pairs, _ = ld_pairs(words, chrom, pos, n, window, max_bp, min_n, min_r2)
    out = [HEADER]
    for p in pairs:
        a, b = cols[int(p["i"])], cols[int(p["j"])]
        out.append("%s\t%s\t%s\t%s\t%s\t%d\t%s\t%s\n" % (a[0], a[1], a[2], b[1], b[2], int(p["n"]), "%.6g" % float(p["r2"]), "+-0"[0 if p["sign"] > 0 else 1 if p["sign"] < 0 else 2]))
    return "".join(out)
