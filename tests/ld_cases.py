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
