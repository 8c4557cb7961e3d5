"""`call --cohort --cohort-priors` and mg_genotype_cohort as far as a machine without a GPU sees them: the definition's numpy form
(tests/cohort_prior_model.py) on cases small enough to work out by hand, the three entries in the header and in the library, and
the command line's errors that come before any device is created.  tests/test_gpu_cohort_priors.py holds the device against the
model; tests/test_gpu_cohort_priors_cli.py runs the command line."""
import os
import subprocess

import numpy as np

from malva_amd import capi

import cohort_prior_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("mg_genotype_cohort", "mg_genotype_cohort_device", "mg_cohort_prior_stats")
E, MAX_COV = 0.001, 200


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).tolist()


# ---- the model on hand-computed cases ---------------------------------------------------------------------------------------------

def test_zero_iterations_is_the_identity():
    for haploid in (False, True):
        cov, freq, vo = M.synth_batch(4, 3, 12, haploid, MAX_COV)
        fo, ni, g1, g2, gq, st, probs, goff = M.genotype_cohort(cov, freq, vo, E, MAX_COV, haploid, 0, 1.0)
        assert bits(fo) == bits(freq) and not ni.any()
        for p in range(3):                                                         # every cell is the single-sample call
            for v in range(12):
                a0, a1 = int(vo[v]), int(vo[v + 1])
                assert (g1[p, v], g2[p, v], gq[p, v], st[p, v]) == M.genotype_cell(cov[p, a0:a1], freq[a0:a1], E, MAX_COV, haploid)[:4]


def test_one_plane_two_alleles_one_iteration_is_the_closed_form():
    """haploid, coverages (1, 1), f0 = (0.75, 0.25): both genotypes have the same binomial and the same read terms, so
    q1 = 0.25^2 / (0.75^2 + 0.25^2) = 0.1, n = 1, and with w = 1: f1 = (0.1 + 1 * 0.25) / (1 * 1 + 1) = 0.175, f0 = 1 - f1.
    Tolerance: the two log priors are floats (2 logf(f), at most 2.8 in size: half an ulp is 1.2e-7), which moves q1 by at most
    q1 (1 - q1) * 2.4e-7 = 2.2e-8 and f1 by half of that; the cast to float adds 7.5e-9: 5e-8 covers it."""
    f, n = M.estimate_record([[1, 1]], [0.75, 0.25], E, MAX_COV, True, 1, 1.0)
    assert n == 1 and f.dtype == np.float32
    assert abs(float(f[1]) - 0.175) <= 5e-8
    assert bits(f[:1]) == bits([np.float32(1.0 - float(f[1]))])                   # the REF rule on the ALT value as stored
    # diploid, coverages (0, 4), f0 = (0.5, 0.5), w = 0: 1/1 has (1-e)^4, 0/1 has 2 * 0.25 * ((1-e)/2)^4 against 0.25 (1-e)^4, 0/0 has e^4:
    # q11 = 1 / (1 + 1/8 + (e / (1-e))^4), q01 = q11 / 8; c1 = q01 + 2 q11; f1 = c1 / 2
    f, n = M.estimate_record([[0, 4]], [0.5, 0.5], E, MAX_COV, False, 1, 0.0)
    q11 = 1.0 / (1.0 + 0.125 + (E / (1 - E)) ** 4)
    assert n == 1 and abs(float(f[1]) - (q11 / 8 + 2 * q11) / 2) <= 2e-7          # (four reads' float terms: 4 * 0.7 * 6e-8 on the exponents, then the cast)


def test_a_plane_that_does_not_count_leaves_n_and_c_untouched():
    alone = M.estimate_record([[3, 5]], [0.9, 0.1], E, MAX_COV, False, 3, 1.0)
    for others in ([[300, 0], [0, 0]], [[0, 0], [0, 201], [0, 0]]):               # over-covered, without coverage
        for at in range(len(others) + 1):
            rows = others[:at] + [[3, 5]] + others[at:]
            f, n = M.estimate_record(rows, [0.9, 0.1], E, MAX_COV, False, 3, 1.0)
            assert n == 1 and bits(f) == bits(alone[0])
    # a covered plane whose every value is 0 (ALT prior 0, 200 reads against REF alone underflow exp): status NORMAL, yet it does not count
    assert M.cell_status([0, 200], MAX_COV) == M.NORMAL and M.expected_copies(np.uint32([0, 200]), np.float32([1, 0]), E, MAX_COV, False)[0] is False
    f, n = M.estimate_record([[0, 200], [3, 5]], [1.0, 0.0], E, MAX_COV, False, 1, 1.0)
    assert n == 1
    f, n = M.estimate_record([[0, 200]], [1.0, 0.0], E, MAX_COV, False, 5, 1.0)
    assert n == 0 and bits(f) == bits([1.0, 0.0])


def test_the_tree_sum_has_its_own_order():
    assert M.tree_sum([1e16, 1.0, -1e16, 1.0], 4) == 2.0                          # (1e16 + -1e16) + (1 + 1); left to right gives 1
    assert M.tree_sum([1e16, 1.0, -1e16], 3) == 1.0                               # padded to four with +0.0
    assert M.tree_sum([0.5], 1) == 0.5 and M.tree_sum([1.0] * 33, 33) == 33.0


def test_the_ref_rule_clamps_at_zero():
    f = M.update([0.0, 3.0, 3.0], 2, np.float32([0.0, 0.5, 0.5]), 2, 0.0)
    assert bits(f) == bits([0.0, 0.75, 0.75])                                      # 1 - 1.5 is negative
    f = M.update([0.0, 1.0], 2, np.float32([0.5, 0.5]), 2, 0.0)
    assert bits(f) == bits([0.75, 0.25])
    f = M.update([0.0, 0.0], 3, np.float32([0.5, 0.5]), 1, 1.0)                   # (0 + 1 * 0.5) / (3 + 1)
    assert bits(f) == bits([0.875, 0.125])


def test_one_allele_and_more_than_eight_are_not_re_estimated():
    for A in (1, 9, 12):
        cov = np.full((4, A), 5, dtype=np.uint32)
        f0 = np.full(A, 1.0 / A, dtype=np.float32)
        f, n = M.estimate_record(cov, f0, E, MAX_COV, False, 5, 1.0)
        assert n == 0 and bits(f) == bits(f0)
    f, n = M.estimate_record(np.full((4, 8), 5, dtype=np.uint32), np.full(8, 0.125, dtype=np.float32), E, MAX_COV, False, 5, 1.0)
    assert n == 4


def test_the_early_stop_changes_nothing():
    cov, freq, vo = M.synth_batch(9, 4, 12, False, MAX_COV)
    a = M.genotype_cohort(cov, freq, vo, E, MAX_COV, False, 64, 0.0)
    b = M.genotype_cohort(cov, freq, vo, E, MAX_COV, False, 64, 0.0, early_stop=False)
    assert bits(a[0]) == bits(b[0]) and a[1].tolist() == b[1].tolist()


# ---- the library and the command line ---------------------------------------------------------------------------------------------

def test_the_library_exports_the_cohort_prior_entries():
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTED and hasattr(L, n), n
    head = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    for n in NAMES:
        assert ("int %s(mg_ctx *ctx" % n) in head, n
    assert "#define MG_PRIOR_MAX_ALLELES 8" in head and "NO reference call" in head and "var_block.hpp:224-330" in head


def _run(args, tmp_path):
    r = subprocess.run([BIN, "call", "-1", "-b", "1"] + args, capture_output=True, text=True, timeout=120)
    assert "HIP device" not in r.stderr and r.stdout == ""
    assert not [n for n in os.listdir(tmp_path) if n not in ("cohort.tsv",)], os.listdir(tmp_path)
    return r


def test_the_errors_that_come_before_any_device(tmp_path):
    fa, vcf, fq = (os.path.join(GOLDEN, n) for n in ("haploid.fa", "haploid.vcf.gz", "haploid.fq"))
    out, table, none = str(tmp_path / "out"), str(tmp_path / "t.tsv"), str(tmp_path / "none.tsv")
    r = _run(["--cohort-priors", fa, vcf, fq], tmp_path)
    assert r.returncode != 0 and "malva : --cohort-priors goes with --cohort" in r.stderr
    r = _run(["--cohort", "-o", out, "--cohort-priors", "--prior-iters", "65", fa, vcf, none], tmp_path)
    assert r.returncode != 0 and "malva : --prior-iters takes a whole number 0..64" in r.stderr
    for bad in ("-1", "x", "5x", ""):
        r = _run(["--cohort", "-o", out, "--cohort-priors", "--prior-iters", bad, fa, vcf, none], tmp_path)
        assert r.returncode != 0 and "--prior-iters" in r.stderr, bad
    for bad in ("-1", "nan", "inf", "1e999", "w", ""):
        r = _run(["--cohort", "-o", out, "--cohort-priors", "--prior-weight", bad, fa, vcf, none], tmp_path)
        assert r.returncode != 0 and "malva : --prior-weight takes a finite number >= 0" in r.stderr, bad
    r = _run(["--cohort", "-o", out, "--priors-out", table, fa, vcf, none], tmp_path)
    assert r.returncode != 0 and "--priors-out go with --cohort-priors" in r.stderr
    for sub in (["--prior-iters", "3"], ["--prior-weight", "2"]):
        r = _run(["--cohort", "-o", out] + sub + [fa, vcf, none], tmp_path)
        assert r.returncode != 0 and sub[0] in r.stderr and "go with --cohort-priors" in r.stderr
    r = _run(["--cohort", "-o", out, "--cohort-priors", "--priors-out", "", fa, vcf, none], tmp_path)
    assert r.returncode != 0 and "malva : --priors-out takes a path" in r.stderr
    # accepted by the usage check: the run gets as far as the manifest, which is missing
    r = _run(["--cohort", "-o", out, "--cohort-priors", "--prior-iters", "0", "--prior-weight", "0", "--priors-out", table, fa, vcf, none], tmp_path)
    assert r.returncode != 0 and "cohort manifest" in r.stderr and "--cohort-priors" not in r.stderr
    # a group below the cohort: refused with the reason once the manifest is read, before any device
    (tmp_path / "cohort.tsv").write_text("a\t%s\nb\t%s\nc\t%s\n" % (fq, fq, fq))
    r = _run(["--cohort", "-o", out, "--cohort-priors", "--cohort-group", "2", "--priors-out", table, fa, vcf, str(tmp_path / "cohort.tsv")], tmp_path)
    assert r.returncode != 0 and "--cohort-group 2" in r.stderr and "--cohort-priors needs the whole cohort in one group" in r.stderr and "3 samples" in r.stderr
    (tmp_path / "cohort.tsv").write_text("".join("s%d\t%s\n" % (i, fq) for i in range(65)))
    r = _run(["--cohort", "-o", out, "--cohort-priors", fa, vcf, str(tmp_path / "cohort.tsv")], tmp_path)
    assert r.returncode != 0 and "at most 64 samples" in r.stderr and "65" in r.stderr


def test_help_lists_the_four_options():
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--cohort-priors", "--prior-iters", "--prior-weight", "--priors-out"):
        line = [l for l in r.stdout.split("\n") if l.lstrip().startswith(opt + " ")]
        assert line, "--help does not list " + opt
    tail = r.stdout[r.stdout.index("--cohort-priors"):r.stdout.index("<kmc_output_prefix>:")]
    assert tail.count("a design choice, not a measurement") == 2 and all(t in tail for t in ("ONE group", "COHORT_AF", "N_INFORMATIVE", "default:5", "default:1"))
