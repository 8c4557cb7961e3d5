"""mg_estimate_priors as far as a machine without a GPU sees it: the wide definition's numpy form (tests/cohort_prior_wide_model.py)
against the one-wave definition it extends (tests/cohort_prior_model.py) and on the seams of the chunked sum, and the three entries
in the header and in the library.  tests/test_gpu_cohort_priors_wide.py holds the device against the model.

The chunked order and one big tree give the same f_T on synthetic cohorts (the float32 cast of the update hides the difference of
the double sums), so nothing here tries to tell the two orders apart through f_T; the sum itself is pinned on values chosen so that
the order shows."""
import os
import subprocess

import numpy as np

from malva_amd import capi

import cohort_prior_model as M
import cohort_prior_wide_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("mg_estimate_priors", "mg_estimate_priors_device", "mg_estimate_priors_stats")
E, MAX_COV = 0.001, 200


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).tolist()


def dbits(x):
    return np.float64(x).view(np.uint64)


def test_up_to_64_planes_it_is_the_one_wave_definition():
    """the sum for every P = 1 .. 64 on values whose low bits differ, and whole records at the segment widths' edges"""
    rng = np.random.default_rng(1)
    vals = rng.random(64) * 10.0 ** rng.integers(-8, 3, 64)
    for P in range(1, 65):
        assert dbits(WM.tree_sum(vals, P)) == dbits(M.tree_sum(vals, P)), P
    for haploid in (False, True):
        for P in (1, 2, 3, 33, 63, 64):
            cov, freq, vo = M.synth_batch(30 + P, P, 12, haploid, MAX_COV)
            for v in range(12):
                a0, a1 = int(vo[v]), int(vo[v + 1])
                f, n = WM.estimate_record(cov[:, a0:a1], freq[a0:a1], E, MAX_COV, haploid, 5, 1.0)
                g, m = M.estimate_record(cov[:, a0:a1], freq[a0:a1], E, MAX_COV, haploid, 5, 1.0)
                assert bits(f) == bits(g) and n == m, (P, v)


def test_the_sum_takes_chunks_of_64_in_order_each_add_rounded():
    """values at which the order shows: 1.0 in plane 0, 2^-53 everywhere else.  Inside a chunk the tree pairs the small values first
    (63 of them reach 1.0 as one term of about 2^-47); across chunks every C_j = 64 * 2^-53 = 2^-47 is added to c on its own."""
    tiny = 2.0 ** -53
    for P in (65, 128, 130, 200):
        vals = [1.0] + [tiny] * (P - 1)
        want = M.tree_sum(vals[:64], 64)
        for lo in range(64, P, 64):
            want = want + M.tree_sum(vals[lo:lo + 64], min(64, P - lo))
        assert dbits(WM.tree_sum(vals, P)) == dbits(want)
    # a short last chunk is padded to its own power of two: the same as padding it to 64, since every value is >= +0.0
    vals = list(np.random.default_rng(2).random(130))
    assert dbits(WM.tree_sum(vals, 130)) == dbits(M.tree_sum(vals[:64], 64) + M.tree_sum(vals[64:128], 64) + M.tree_sum(vals[128:] + [0.0] * 62, 64))
    # the sum is not the left-to-right one (the definition is the tree)
    left = 0.0
    for x in [1.0] + [tiny] * 63:
        left = left + x
    assert left == 1.0 and WM.tree_sum([1.0] + [tiny] * 63, 64) > 1.0


def test_a_whole_chunk_of_planes_that_do_not_count_leaves_c_and_n():
    cov, freq, vo = M.synth_batch(7, 64, 12, False, MAX_COV)
    dead = np.zeros((64, cov.shape[1]), dtype=np.uint32)                             # a chunk without coverage
    over = np.full((64, cov.shape[1]), MAX_COV + 1, dtype=np.uint32)                 # a chunk over-covered
    base = WM.estimate_priors(cov, freq, vo, E, MAX_COV, False, 5, 1.0)
    assert base[1].max() > 32
    for stack in ([cov, dead], [dead, cov], [over, cov, dead], [cov, over[:5]]):
        got = WM.estimate_priors(np.concatenate(stack), freq, vo, E, MAX_COV, False, 5, 1.0)
        assert bits(got[0]) == bits(base[0]) and np.array_equal(got[1], base[1])


def test_plane_64_as_the_only_plane_that_counts():
    for haploid in (False, True):
        alone = M.estimate_record([[3, 5]], [0.9, 0.1], E, MAX_COV, haploid, 3, 1.0)
        rows = [[0, 0]] * 32 + [[MAX_COV + 1, 0]] * 32 + [[3, 5]] + [[0, 0]] * 2
        f, n = WM.estimate_record(rows, [0.9, 0.1], E, MAX_COV, haploid, 3, 1.0)
        assert n == 1 and alone[1] == 1 and bits(f) == bits(alone[0]) and bits(f) != bits([0.9, 0.1])


def test_no_plane_counts_over_all_chunks_keeps_f():
    for rows in ([[0, 0]] * 130, [[MAX_COV + 1, 1]] * 65, [[0, 0]] * 64 + [[0, MAX_COV + 7]] * 64 + [[0, 0]]):
        f, n = WM.estimate_record(rows, [0.9, 0.1], E, MAX_COV, False, 5, 1.0)
        assert n == 0 and bits(f) == bits([0.9, 0.1])
    # records that are not re-estimated: A = 1, A = 9, T = 0
    cov, freq, vo = M.synth_batch(9, 66, 12, False, MAX_COV)
    fo, ni = WM.estimate_priors(cov, freq, vo, E, MAX_COV, False, 0, 1.0)
    assert bits(fo) == bits(freq) and not ni.any()
    fo, ni = WM.estimate_priors(cov, freq, vo, E, MAX_COV, False, 5, 1.0)
    A = np.diff(vo.astype(np.int64))
    for v in np.flatnonzero((A < 2) | (A > 8)):
        assert bits(fo[vo[v]:vo[v + 1]]) == bits(freq[vo[v]:vo[v + 1]]) and ni[v] == 0
    assert ni.max() > 32 and bits(fo) != bits(freq)


def test_record_ranges_give_the_same_arrays():
    cov, freq, vo = M.synth_batch(11, 70, 24, True, MAX_COV)
    fo, ni = WM.estimate_priors(cov, freq, vo, E, MAX_COV, True, 5, 1.0)
    for cuts in ((0, 24), (0, 16, 24), (0, 17, 24), (0, 1, 7, 8, 24)):
        f_parts, n_parts = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            c, f, o = WM.record_range(cov, freq, vo, lo, hi)
            assert c.shape == (70, int(o[-1])) and o[0] == 0
            a, b = WM.estimate_priors(c, f, o, E, MAX_COV, True, 5, 1.0)
            f_parts.append(a)
            n_parts.append(b)
        assert bits(np.concatenate(f_parts)) == bits(fo) and np.array_equal(np.concatenate(n_parts), ni), cuts


def test_the_library_exports_the_estimate_entries():
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTED and hasattr(L, n), n
    head = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    for n in NAMES:
        assert ("int %s(mg_ctx *ctx" % n) in head, n
    assert "#define MG_PRIOR_WIDE_MAX_PLANES 16384" in head and WM.MAX_PLANES == 16384 and "a design choice" in head
    assert "padding\n * a short chunk to 64 lanes gives the same C_j" in head


def test_prior_groups_goes_with_cohort_priors(tmp_path):
    """refused with the options, before any device is created; nothing is written.  --help lists it with its disk need and its limit"""
    fa, vcf = (os.path.join(GOLDEN, n) for n in ("haploid.fa", "haploid.vcf.gz"))
    out, none = str(tmp_path / "out"), str(tmp_path / "none.tsv")
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "-o", out, "--prior-groups", fa, vcf, none], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "malva : --prior-groups goes with --cohort-priors" in r.stderr and "HIP device" not in r.stderr and r.stdout == ""
    assert not os.listdir(str(tmp_path))
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and [l for l in r.stdout.split("\n") if l.lstrip().startswith("--prior-groups ")]
    tail = r.stdout[r.stdout.index("--prior-groups"):r.stdout.index("--prior-iters")]
    assert all(t in tail for t in ("4 B x allele slots x samples", "16384", "65536", "8192", "$TMPDIR"))
