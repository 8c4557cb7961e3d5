"""The case table of the LD tests (tests/test_ld_cases_cpu.py proves what each case says of itself, tests/test_gpu_ld.py runs them on
the device).  A directed case is a dict: name, words [groups, 3, n_vars], chrom, pos, params (n_first, window, max_bp, min_n, min_r2),
pair (i, j) and `says`: "emitted", or the one rule of ld_model.RULES that alone keeps the pair out; `sign` where the case is about it."""
import numpy as np

from ld_model import pair_value, words_from_dosage

MISSING = -1


def _case(name, D, says, pair=(0, 1), chrom=None, pos=None, group_sizes=None, sign=None, **params):
    D = np.asarray(D, dtype=np.int64)
    n = D.shape[0]
    p = dict(n_first=n, window=4, max_bp=0, min_n=1, min_r2=0.0)
    p.update(params)
    return dict(name=name, words=words_from_dosage(D, group_sizes), chrom=np.zeros(n, dtype=np.uint32) if chrom is None else np.asarray(chrom, dtype=np.uint32),
                pos=np.arange(100, 100 + 10 * n, 10, dtype=np.uint32) if pos is None else np.asarray(pos, dtype=np.uint32), params=p, pair=pair, says=says, sign=sign)


def big_dosage():
    """16,384 samples (256 groups of 64), two records: three classes at uneven frequencies, the second record the first one's with one
    cell in ten redrawn, a few hundred cells of each missing"""
    rng = np.random.default_rng(64)          # (a seed under which neither product is a double: test_ld_cases_cpu.py)
    S = 16384
    x = rng.choice(3, size=S, p=[0.41, 0.37, 0.22])
    y = np.where(rng.random(S) < 0.1, rng.choice(3, size=S, p=[0.3, 0.3, 0.4]), x)
    x, y = x.astype(np.int64), y.astype(np.int64)
    x[rng.choice(S, 301, replace=False)] = MISSING
    y[rng.choice(S, 457, replace=False)] = MISSING
    return np.stack([x, y])


X025, Y025 = (0, 0, 1), (0, 1, 1)        # cov = 1, vx = vy = 2: r2 = 1 / 4 exactly
BASE = np.array([[0, 0, 1, 2, 1], [0, 1, 1, 2, 0]])     # an ordinary pair: both vary, cov > 0


def directed_cases():
    out = []
    out.append(_case("wide: both products beyond 2^53 and not representable, 256 groups", big_dosage(), "emitted", min_r2=0.2, min_n=2))
    out.append(_case("r2 exactly min_r2 = 0.25: emitted", [X025, Y025], "emitted", min_r2=0.25, sign=1))
    r2 = pair_value(words_from_dosage(BASE), 0, 1)[4]
    out.append(_case("r2 exactly min_r2, an ordinary value", BASE, "emitted", min_r2=r2, sign=1))
    out.append(_case("r2 one ulp below min_r2", BASE, "min_r2", min_r2=float(np.nextafter(r2, 2.0))))
    out.append(_case("vx == 0: the first record does not vary", [[1, 1, 1, 1, 1], BASE[1]], "vx"))
    out.append(_case("vy == 0: the second record does not vary", [BASE[0], [2, 2, 2, 2, 2]], "vy"))
    out.append(_case("the sums run over the shared samples alone", [[0, 1, 1, 1, MISSING], [0, MISSING, 1, 2, 1]], "emitted", sign=1))
    out.append(_case("vx == 0 among the shared samples only, rejected", [[0, 1, 1, 1, 2], [MISSING, 0, 1, 2, MISSING]], "vx"))
    out.append(_case("n < min_n", BASE, "min_n", min_n=6))
    out.append(_case("n == min_n", BASE, "emitted", min_n=5))
    out.append(_case("contig change", BASE, "chrom", chrom=[0, 1]))
    out.append(_case("max_bp: one base too far", BASE, "max_bp", pos=[100, 151], max_bp=50))
    out.append(_case("max_bp: the last base inside", BASE, "emitted", pos=[100, 150], max_bp=50))
    out.append(_case("max_bp: positions that descend, one base too far", BASE, "max_bp", pos=[4000000000, 3999999949], max_bp=50))
    out.append(_case("max_bp: the whole range of a position", BASE, "emitted", pos=[0, 0xFFFFFFFF], max_bp=0xFFFFFFFF))
    far = np.stack([BASE[0], [0] * 5, [0] * 5, [0] * 5, BASE[1]])
    out.append(_case("beyond the window", far, "window", pair=(0, 4), window=3))
    out.append(_case("the window's last record", far, "emitted", pair=(0, 4), window=4))
    out.append(_case("i >= n_first: a partner only", np.stack([BASE[0], BASE[0], BASE[1]]), "n_first", pair=(1, 2), n_first=1))
    out.append(_case("cov < 0", [BASE[0], 2 - BASE[1]], "emitted", sign=-1))
    out.append(_case("cov == 0 with both varying: r2 = 0 >= min_r2 = 0", [[0, 0, 1, 1], [0, 1, 0, 1]], "emitted", sign=0))
    out.append(_case("cov > 0, r2 = 1", [[0, 1, 2, MISSING], [0, 1, 2, 2]], "emitted", sign=1, min_r2=1.0))
    out.append(_case("samples of two groups, one cell each", [[0, 1, 2], [0, 1, 2]], "emitted", group_sizes=[1, 2], sign=1, min_r2=1.0))
    return out


def group_sizes_for(n_groups):
    """planes per group: full, ragged, one plane; two planes each in the wide case (so that its restatement stays small)"""
    return {1: [64], 2: [64, 37], 3: [64, 1, 63], 17: [3] * 16 + [64], 256: [2] * 256}[n_groups]


def random_dosage(n_vars, samples, run, seed):
    """records in runs of `run` that share a latent record, one cell in five redrawn: r2 around 0.4 inside a run, around 0 across; one
    cell in ten missing, one record in ten without cells (not biallelic)"""
    rng = np.random.default_rng(seed)
    n_lat = n_vars // run + 2
    latent = rng.choice(3, size=(n_lat, samples), p=[0.5, 0.3, 0.2])
    D = latent[np.arange(n_vars) // run]
    redraw = rng.random((n_vars, samples)) < 0.2
    D = np.where(redraw, rng.choice(3, size=(n_vars, samples)), D).astype(np.int64)
    D[rng.random((n_vars, samples)) < 0.1] = MISSING
    D[rng.random(n_vars) < 0.1] = MISSING
    return D


def window_case(window, n_vars, n_groups):
    """-> (words, chrom, pos, max_bp): a random table of n_vars records over n_groups groups: three contigs and one of a single record
    between them (where n_vars allows), positions ascending inside a contig by 1..200, and a max_bp that cuts windows short"""
    sizes = group_sizes_for(n_groups)
    seed = window * 100003 + n_vars * 101 + n_groups
    D = random_dosage(n_vars, sum(sizes), max(2, window // 2), seed)
    rng = np.random.default_rng(seed + 1)
    chrom = np.zeros(n_vars, dtype=np.uint32)
    for cut in (n_vars // 3, n_vars // 3 + 1, 2 * n_vars // 3):
        if 0 < cut < n_vars:
            chrom[cut:] += 1
    pos = np.cumsum(rng.integers(1, 201, size=n_vars)).astype(np.uint32)
    for arr in (chrom, pos):
        arr.setflags(write=False)
    words = words_from_dosage(D, sizes) if n_vars else np.zeros((n_groups, 3, 0), dtype=np.uint64)
    words.setflags(write=False)
    return words, chrom, pos, 25 * window + 50


WINDOWS = (1, 3, 64, 1024)
GROUPS = (1, 2, 3, 256)


def n_vars_for(window):
    return sorted({0, 1, 2, window, window + 1, window + 66, 257})


# ---- seam cases: the geometry of ld_window_kernel and pack_site_kernel ------------------------------------------------------------------
# A seam case is a table in which every record is monomorphic (all samples of all groups called with dosage 0: vx == 0 or vy == 0 keeps
# every pair with it out) except the records it names.  A named record carries five cells, dosages PATTERNS[k], in bits `bit0 ..` of ONE
# group and no other cell.  So the emitted pairs are exactly the pairs of named records of one group that the rules let through, and the
# case says which: `pairs` the whole set, `present` / `absent` the ones it is about (absent with the one rule that rejects them).
# `decoys` are named records of their own -- the same cells one group and one dosage row off, or one record beyond a limit: they share no
# sample with the records beside them (n == 0) or lie where a rule rejects them, so a read that is one off turns an absence into a presence;
# tests/test_ld_cases_cpu.py proves that the table without them gives the same pairs.
LD_R, LD_TILE, LD_JN, LD_GC, SCAN_CHUNK = 4, 16, 80, 16, 8192            # ld_kernels.h, the library's scan (a test's copy)
PATTERNS = ((0, 0, 1, 2, 1), (0, 1, 1, 2, 0), (2, 1, 0, 0, 1))
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _seam_words(n_vars, n_groups, named, bit0=0):
    """named: {record: (group, pattern index)} -> uint64 [n_groups, 3, n_vars]"""
    w = np.zeros((n_groups, 3, n_vars), dtype=np.uint64)
    w[:, 0, :] = ALL_ONES
    for v, (g, k) in named.items():
        w[:, :, v] = 0
        for s, d in enumerate(PATTERNS[k % 3]):
            w[g, d, v] |= np.uint64(1) << np.uint64(bit0 + s)
    return w


def _seam(name, n_vars, window, named, present, absent=(), decoys=None, n_first=None, n_groups=1, group=0, caps=(), seams=()):
    """named: record indexes (group `group`, patterns in turn); decoys: {record: (group, pattern index)}"""
    n_first = n_vars if n_first is None else n_first
    mine = {v: (group, k) for k, v in enumerate(sorted(named))}
    decoys = dict(decoys or {})
    assert not set(mine) & set(decoys)
    both = {**mine, **decoys}
    pairs = sorted((a, b) for a in both for b in both if a < b <= a + window and a < n_first and both[a][0] == both[b][0])
    p = dict(n_first=n_first, window=window, max_bp=0, min_n=1, min_r2=0.0)
    case = dict(name=name, words=_seam_words(n_vars, n_groups, both), plain=_seam_words(n_vars, n_groups, mine), chrom=np.zeros(n_vars, dtype=np.uint32),
                pos=np.arange(100, 100 + 10 * n_vars, 10, dtype=np.uint32), params=p, pairs=pairs, present=list(present), absent=list(absent), decoys=decoys,
                caps=list(caps), seams=set(seams))
    for x in (case["words"], case["plain"], case["chrom"], case["pos"]):
        x.setflags(write=False)
    return case


def tile_place(i, j):
    """where the kernel meets the pair: (ir, slab, lane, jr) -- i's row in its tile, the slab of the offset, the lane, the partner's index in
    the slab's partner run"""
    off = j - i
    ir, slab, lane = i % LD_TILE, (off - 1) // 64, (off - 1) % 64
    return ir, slab, lane, ir + lane


def _rows_before(pairs, i):
    return sum(1 for a, _ in pairs if a < i)


def seam_cases():
    out = []
    # ---- the window's end inside a later slab: (i, i + window) is the last pair, (i, i + window + 1) none; partners at 64, 65, 128, 129, 64 k + 63
    for W in (63, 65, 127, 128, 129, 1023):
        offs = sorted({o for o in [1, 64, 65, 128, 129, W - 1, W, W + 1] + [64 * k + 63 for k in range(16)] if 1 <= o <= W + 1})
        named = [5] + [5 + o for o in offs]
        out.append(_seam("window_%d" % W, 5 + W + 5, W, named, present=[(5, 5 + o) for o in offs if o <= W], absent=[(5, 5 + W + 1, "window")], seams={"window_%d" % W}))
    # ---- record i at the seams of a wave's LD_R and a workgroup's LD_TILE, the partner at jr 0, 63, 64, 78 of the partner run
    spots = [(16, 1), (32, 65), (3, 61), (4, 61), (17, 64), (15, 64), (31, 128), (16, 64), (31, 64)]
    named = sorted({i for i, _ in spots} | {i + o for i, o in spots})
    out.append(_seam("rows_of_a_tile", 200, 128, named, present=[(i, i + o) for i, o in spots], absent=[(31, 31 + 129, "window")], decoys={160: (0, 1)},
                     seams={"tile_rows"}))
    # ---- the ends of the table
    out.append(_seam("partner_is_the_last_record", 40, 64, [0, 10, 39], present=[(10, 39), (0, 39)], absent=[(10, 40, "n_vars")], seams={"last_record"}))
    out.append(_seam("last_tile_has_no_partner", 33, 64, [30, 32], present=[(30, 32)], absent=[(32, 33, "n_vars")], seams={"empty_tile"}))
    out.append(_seam("a_later_slab_starts_beyond_the_table", 70, 200, [0, 2, 69], present=[(0, 2), (0, 69), (2, 69)], absent=[(2, 70, "n_vars")], seams={"slab_beyond"}))
    # ---- n_first below n_vars: record n_first - 1 is kept, record n_first is a partner only
    for nf in (1, 15, 16, 17, 33):
        out.append(_seam("n_first_%d" % nf, nf + 6, 4, [nf - 1, nf, nf + 1], present=[(nf - 1, nf), (nf - 1, nf + 1)], absent=[(nf, nf + 1, "n_first")], n_first=nf,
                         seams={"n_first_%d" % nf}))
    # ---- the groups: the chunk of LD_GC = 16 and the ragged last chunk; the only samples that vary live in one group
    for G, g in ((15, 0), (16, 15), (17, 15), (17, 16), (32, 31), (33, 16), (33, 31), (33, 32)):
        decoys = {3: ((g + 1) % G, 1), 6: ((g - 1) % G, 2), 8: ((g + 1) % G, 0)}   # beside record 2, beside record 5, alone: one group and one dosage row off
        out.append(_seam("groups_%d_vary_in_%d" % (G, g), 12, 4, [2, 5], present=[(2, 5)], absent=[(2, 3, "min_n"), (5, 6, "min_n"), (3, 6, "min_n")], decoys=decoys, n_groups=G,
                         group=g, seams={"groups_%d" % G, "vary_in_%d" % g}))
    # ---- write positions: pairs in slab 0, none in slab 1, some in slab 2; lanes 0, 31, 32, 63 of both; two records of one wave with
    # different counts; pairs_cap inside the ballot of slab 0 and of slab 2
    offs = [1, 32, 33, 64, 129, 160, 161, 192]
    named = [5] + [5 + o for o in offs]
    c = _seam("write_positions", 210, 192, named, present=[(5, 5 + o) for o in offs] + [(6, 37), (6, 197)], absent=[(5, 198, "window")], seams={"write_positions"})
    before = _rows_before(c["pairs"], 5)
    c["caps"] = [before + 2, before + 6, before + 8]
    out.append(c)
    # ---- row_off across a part of the library's scan: n_first = SCAN_CHUNK + 1, window 1, one group
    n = SCAN_CHUNK + 3
    out.append(_seam("n_first_8193", n, 1, [0, 1, 8191, 8192, 8193, 8194], present=[(0, 1), (8191, 8192), (8192, 8193)], absent=[(8193, 8194, "n_first")],
                     n_first=SCAN_CHUNK + 1, seams={"scan_chunk"}))
    assert len({c["name"] for c in out}) == len(out)
    return out


LD_SEAMS = ({"window_%d" % w for w in (63, 65, 127, 128, 129, 1023)} | {"tile_rows", "last_record", "empty_tile", "slab_beyond", "write_positions", "scan_chunk"} |
            {"n_first_%d" % n for n in (1, 15, 16, 17, 33)} | {"groups_%d" % g for g in (15, 16, 17, 32, 33)} | {"vary_in_%d" % g for g in (0, 15, 16, 31, 32)})

# pack_site_kernel: one called cell among cells that look called but are masked out, one plane and one record off included
PACK_PLANES, PACK_RECORDS, PACK_N, PACK_MIN_GQ = (0, 3, 4, 5, 62, 63), (0, 63, 64, 129), 130, 30


def pack_case(plane, record, dosage):
    """-> (g1, g2, gq, vao): 64 planes x 130 records; every cell is 1/1 with GQ one below the mask -- a decoy -- but the cell (plane, record),
    which has the dosage and GQ exactly at the mask"""
    g1, g2 = np.ones((64, PACK_N), dtype=np.int32), np.ones((64, PACK_N), dtype=np.int32)
    gq = np.full((64, PACK_N), PACK_MIN_GQ - 1, dtype=np.int32)
    g1[plane, record], g2[plane, record], gq[plane, record] = dosage // 2, (dosage + 1) // 2, PACK_MIN_GQ
    return g1, g2, gq, np.arange(0, 2 * PACK_N + 1, 2, dtype=np.uint32)


def pack_cases():
    return [(p, v, (p + v) % 3) for p in PACK_PLANES for v in PACK_RECORDS]
