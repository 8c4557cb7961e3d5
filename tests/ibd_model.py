"""A plain restatement of the IBS0-free segments (`call --cohort --ibd`, mg_ibd_begin / mg_ibd_step in include/malva_hip.h): the walk of
every pair of samples along the records, record by record in the order the definition gives, and the table's text from a parsed merged
VCF.  The pairs are numpy vectors, the records a Python loop; every value is an integer, so the device, the host and this file agree
exactly."""
import numpy as np

from ld_model import parse_merged_vcf, site_words

IBD_SEG = np.dtype([(f, np.uint32) for f in ("a", "b", "chrom", "start_pos", "end_pos", "n", "ibs2", "zero")])
HEADER = "#A\tB\tCHROM\tSTART\tEND\tLENGTH\tN\tIBS2\n"


def dosage_from_words(words, n_samples):
    """uint64 [groups, 3, n_vars] -> int64 [n_vars, n_samples]: the cell's dosage, -1 where it does not contribute; sample 64 g + p is
    bit p of group g"""
    words = np.asarray(words, dtype=np.uint64)
    G, three, n = words.shape
    assert three == 3 and G == (n_samples + 63) // 64
    D = np.full((n, n_samples), -1, dtype=np.int64)
    for s in range(n_samples):
        g, p = divmod(s, 64)
        for d in range(3):
            D[(words[g, d] >> np.uint64(p)) & np.uint64(1) == 1, s] = d
    return D


def planes_from_words(words):
    """uint64 [groups, 3, n_vars] -> uint64 [64 groups, 3, W], mg_pack_dosage's layout: bit v & 63 of word v >> 6 of [64 g + p, d] is bit
    p of words[g, d, v]"""
    words = np.asarray(words, dtype=np.uint64)
    G, _, n = words.shape
    W = (n + 63) // 64
    out = np.zeros((64 * G, 3, W), dtype=np.uint64)
    v = np.arange(n)
    for g in range(G):
        for d in range(3):
            for p in range(64):
                bits = (words[g, d] >> np.uint64(p)) & np.uint64(1)
                np.bitwise_or.at(out[64 * g + p, d], v >> 6, bits << (v & 63).astype(np.uint64))
    return out


class IbdModel:
    """the state of all pairs a < b of n_samples samples, ordered by a, then b; step() takes the next records"""

    def __init__(self, n_samples, min_records, min_bp):
        assert n_samples >= 2 and min_records >= 1 and min_bp >= 0
        self.n_samples, self.min_records, self.min_bp = n_samples, min_records, min_bp
        self.a, self.b = np.triu_indices(n_samples, 1)                  # (row-major: by a, then b)
        P = self.a.size
        self.open = np.zeros(P, dtype=bool)
        self.chrom, self.start, self.end, self.n, self.ibs2 = (np.zeros(P, dtype=np.int64) for _ in range(5))
        self.filtered = {"min_records": 0, "min_bp": 0}                  # closed runs each threshold kept out of the table

    def _close(self, which, out):
        """close the open states among `which` (a mask); the emitted ones are appended to out"""
        which = which & self.open
        if not which.any():
            return
        idx = np.nonzero(which)[0]
        enough = self.n[idx] >= self.min_records
        long_enough = self.end[idx] - self.start[idx] >= self.min_bp    # (int64)
        self.filtered["min_records"] += int((~enough).sum())
        self.filtered["min_bp"] += int((~long_enough).sum())
        keep = idx[enough & long_enough]
        out.append((keep, self.chrom[keep], self.start[keep], self.end[keep], self.n[keep], self.ibs2[keep]))
        self.open[idx] = False

    def step(self, D, chrom, pos, flush=False):
        """D int [n_vars, n_samples] (a dosage, or -1), chrom / pos [n_vars] -> the segments closed in this step, IBD_SEG ordered by (a, b)
        and along the records"""
        D = np.asarray(D, dtype=np.int64).reshape(-1, self.n_samples)
        chrom, pos = np.asarray(chrom, dtype=np.int64), np.asarray(pos, dtype=np.int64)
        out = []
        for v in range(D.shape[0]):
            da, db = D[v, self.a], D[v, self.b]
            both = (da >= 0) & (db >= 0)
            disc = both & (np.abs(da - db) == 2)
            conc = both & ~disc
            self._close(self.chrom != chrom[v], out)                    # 1. another chromosome
            self._close(disc, out)                                      # 2. DISC
            opens = conc & ~self.open                                   # 3. CONC
            self.open[opens] = True
            self.chrom[opens], self.start[opens], self.n[opens], self.ibs2[opens] = chrom[v], pos[v], 0, 0
            self.end[conc] = pos[v]
            self.n[conc] += 1
            self.ibs2[conc & (da == db)] += 1
        if flush:
            self._close(np.ones(self.a.size, dtype=bool), out)
        if not out:
            return np.zeros(0, dtype=IBD_SEG)
        pair = np.concatenate([o[0] for o in out])
        order = np.argsort(pair, kind="stable")                         # by (a, b); within a pair the order of closing
        seg = np.zeros(pair.size, dtype=IBD_SEG)
        seg["a"], seg["b"] = self.a[pair][order], self.b[pair][order]
        for i, f in enumerate(("chrom", "start_pos", "end_pos", "n", "ibs2")):
            seg[f] = np.concatenate([o[i + 1] for o in out])[order]
        return seg


def sort_segments(parts):
    """the steps' outputs, in step order -> one table ordered by (a, b) and along the records: a stable sort by (a, b)"""
    parts = [p for p in parts if len(p)]
    if not parts:
        return np.zeros(0, dtype=IBD_SEG)
    seg = np.concatenate(parts)
    key = seg["a"].astype(np.int64) << 32 | seg["b"].astype(np.int64)
    return seg[np.argsort(key, kind="stable")]


def ibd_segments(D, chrom, pos, n_samples, min_records, min_bp, cuts=(), flush=True, model=None):
    """the whole table of a walk cut at the record indexes `cuts` (each cut starts a new step; the last step flushes)"""
    D = np.asarray(D, dtype=np.int64).reshape(-1, n_samples)
    m = model or IbdModel(n_samples, min_records, min_bp)
    edges = [0] + sorted(cuts) + [D.shape[0]]
    parts = []
    for i, (c0, c1) in enumerate(zip(edges[:-1], edges[1:])):
        parts.append(m.step(D[c0:c1], chrom[c0:c1], pos[c0:c1], flush=flush and i == len(edges) - 2))
    return sort_segments(parts)


# ---- the table of the command line ------------------------------------------------------------------------------------------------

def ibd_table_text(vcf_text, min_records=100, min_bp=1000000, min_gq=None, group=64):
    """the bytes `--ibd PATH` holds for the merged VCF a run wrote"""
    names = next(l for l in vcf_text.split("\n") if l.startswith("#CHROM")).split("\t")[9:]
    cols, g1, g2, gq, vao, haploid = parse_merged_vcf(vcf_text)
    n, S = len(cols), g1.shape[0]
    assert S == len(names)
    words = np.stack([site_words(g1[s:s + group], g2[s:s + group], gq[s:s + group], haploid, vao, min_gq) for s in range(0, S, group)])
    D = np.concatenate([dosage_from_words(words[g:g + 1], min(group, S - g * group)) for g in range(words.shape[0])], axis=1)
    chrom, last, chrom_names = np.zeros(n, dtype=np.int64), None, []
    for v, c in enumerate(cols):                 # a running id that steps whenever the CHROM text changes
        if c[0] != last:
            chrom_names.append(c[0])
        chrom[v] = len(chrom_names) - 1
        last = c[0]
    pos = np.array([int(c[1]) for c in cols], dtype=np.int64)
    out = [HEADER]
    for s in ibd_segments(D, chrom, pos, S, min_records, min_bp):
        out.append("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (names[int(s["a"])], names[int(s["b"])], chrom_names[int(s["chrom"])], int(s["start_pos"]), int(s["end_pos"]),
                                                     int(s["end_pos"]) - int(s["start_pos"]), int(s["n"]), int(s["ibs2"])))
    return "".join(out)
