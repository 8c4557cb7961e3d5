"""The directed cases of the genetic relationship matrix (tests/grm_model.py restates the definition).  A case is a dict: name, n_samples, D
(int64 [n_vars, n_samples]: the cells' dosages, -1 where a cell does not contribute), haploid, maf_ppm, min_n, and `enters`: which records
enter, as the case CLAIMS it (None: the case claims nothing about it) -- tests/test_grm_cases_cpu.py proves the claims against the model
without a GPU, tests/test_gpu_grm.py runs the device over the same table."""
import numpy as np

import grm_model as M


def _case(name, D, n_samples, enters=None, haploid=False, maf_ppm=0, min_n=1, **more):
    D = np.asarray(D, dtype=np.int64).reshape(-1, n_samples)
    D.setflags(write=False)
    return dict(name=name, D=D, n_samples=n_samples, enters=None if enters is None else list(enters), haploid=haploid, maf_ppm=maf_ppm, min_n=min_n, **more)


def _one_alt(n, alt=2, ref=0):
    """one record: sample 0 has dosage `alt`, the other n - 1 samples `ref`"""
    row = np.full(n, ref, dtype=np.int64)
    row[0] = alt
    return row


def _by_counts(n_samples, n0, n1, n2):
    """one record with these counts, the rest not contributing; the dosages interleaved so that neighbours differ"""
    row = np.full(n_samples, -1, dtype=np.int64)
    cells = np.array([0] * n0 + [1] * n1 + [2] * n2, dtype=np.int64)
    row[np.random.default_rng(n0 * 1000003 + n1 * 1009 + n2).permutation(n_samples)[:cells.size]] = cells
    return row


def random_dosage(n_vars, n_samples, seed, missing=0.1):
    """cells with an allele frequency of their record and a call rate of their sample: no two samples alike"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.03, 0.97, size=(n_vars, 1))
    D = (rng.random((n_vars, n_samples)) < p).astype(np.int64) + (rng.random((n_vars, n_samples)) < p)
    rate = rng.uniform(0.0, 2 * missing, size=(1, n_samples))
    D[rng.random((n_vars, n_samples)) < rate] = -1
    return D


def digit_extremes(limit=60):
    """records (n0, n1, n2), n <= limit, whose weights hold a digit at its extreme: l = 127, l = -128, found by the model.  h = 127 and
    h = -127 come from the |q| boundary (q = 32608 and -32608).  h = -128 cannot occur: it needs q <= -32641, beyond MG_GRM_MAX_Q."""
    want = {}
    for n in range(2, limit + 1):
        for n1 in range(n + 1):
            n2 = np.arange(0, n - n1 + 1)
            q, enters = M.weights_from_counts(n - n1 - n2, np.full_like(n2, n1), n2)
            h, l = M.digits(q)
            for key, hit in (("l=127", l == 127), ("l=-128", l == -128)):
                hit = hit.any(axis=1) & enters
                if key not in want and hit.any():
                    k = int(n2[np.argmax(hit)])
                    want[key] = (n - n1 - k, n1, k)
        if len(want) == 2:
            break
    return want


SAMPLE_COUNTS = [1, 2, 15, 16, 17, 31, 33, 64, 65, 130]
RECORD_COUNTS = [0, 1, 63, 64, 65, 4097]
FOLD_SAMPLES, FOLD_RECORDS = 508, 140000


def directed_cases():
    out = []
    # the |q| boundary: one hom-alt sample among n hom-ref ones, q2 = 1024 sqrt(2 (n - 1)): 32608 at 508, beyond MG_GRM_MAX_Q from 509 on
    out.append(_case("q_boundary_508_enters", [_one_alt(508), _one_alt(508, alt=0, ref=2)], 508, enters=[True, True], q_first=(-64, 16272, 32608)))
    out.append(_case("q_boundary_509_does_not", [_one_alt(509), _one_alt(509, alt=0, ref=2)], 509, enters=[False, False]))
    out.append(_case("q_boundary_600_does_not", [_one_alt(600)], 600, enters=[False]))
    # the MAF threshold: 100 samples, AN = 200, 5 %: AC = 10 is at it, AC = 9 one count below; the same from the other side
    maf = [_by_counts(100, 90, 10, 0), _by_counts(100, 91, 9, 0), _by_counts(100, 0, 10, 90), _by_counts(100, 0, 9, 91), _by_counts(100, 95, 0, 5)]
    out.append(_case("maf_at_and_below", maf, 100, enters=[True, False, True, False, True], maf_ppm=50000))
    # min_n: exactly at it and one below
    out.append(_case("min_n_at_and_below", [_by_counts(40, 6, 3, 1), _by_counts(40, 5, 3, 1), _by_counts(40, 30, 6, 4)], 40, enters=[True, False, True], min_n=10))
    # records that never enter: monomorphic both ways, all cells missing, all heterozygous is NOT one of them (AC = n: p = 0.5)
    never = [np.zeros(20, dtype=np.int64), np.full(20, 2), np.full(20, -1), np.full(20, 1), _by_counts(20, 10, 5, 5)]
    out.append(_case("never_enter", never, 20, enters=[False, False, False, True, True]))
    # a multi-allelic record has no bits at all: it is an all-missing record among biallelic ones
    rows = random_dosage(9, 33, seed=5)
    rows[[2, 6]] = -1
    out.append(_case("multiallelic_among_biallelic", rows, 33, enters=None, no_bits=[2, 6]))
    # haploid: dosages 0 and 2; a dosage-1 bit is ignored
    hap = random_dosage(40, 70, seed=6)
    hap[hap == 1] = 2
    hap[3, :5] = 1
    out.append(_case("haploid", hap, 70, haploid=True))
    out.append(_case("haploid_maf_and_min_n", hap, 70, haploid=True, maf_ppm=200000, min_n=60))
    # digits at their extremes
    ext = digit_extremes()
    n = max(sum(c) for c in ext.values())
    out.append(_case("digit_extremes", [_by_counts(n, *ext["l=127"]), _by_counts(n, *ext["l=-128"])], n, enters=[True, True], digits=ext))
    # sample counts around the tiles and the words; the spare bits of the last group are set in the words (words_from_dosage)
    for s in SAMPLE_COUNTS:
        out.append(_case("samples_%d" % s, random_dosage(50, s, seed=100 + s), s, maf_ppm=10000 if s > 2 else 0, min_n=2 if s > 1 else 1))
    # record counts around the MFMA's K and a step of several runs
    for r in RECORD_COUNTS:
        out.append(_case("records_%d" % r, random_dosage(r, 33, seed=200 + r), 33, maf_ppm=10000, min_n=2))
    return out


def fold_case():
    """508 samples, 140,000 identical records, sample 0 hom-alt and the rest hom-ref: h h = 16129 a record, past 2^31 from 133,145 records on.
    -> (one record's D, the number of records)"""
    return _one_alt(FOLD_SAMPLES).reshape(1, -1), FOLD_RECORDS


# ---- the run plan: the Gram kernel without atomics, and a full run of the i32 accumulators ---------------------------------------------
# A plan case is a dict: name, n_samples, front (random records, no two samples alike, or None), record (one record's dosages) and count
# (how often it follows the front), and `plan`: the pieces mg_grm_step must cut the one step into, as (records, run, runs) -- runs == 1 is
# grm_gram_kernel<false>.  tests/test_grm_cases_cpu.py proves the plan from the restatement of tests/test_grm_plan_cpu.py, which that file
# holds against csrc/grm_plan.h.
BOUND_SAMPLES, BOUND_ALT = 2017, (0, 31, 32, 2016)          # 64 blocks of 32: 2,080 on and above the diagonal, the first count past GRM_FILL
BOUND_Q, BOUND_H = (-65, 16211, 32487), 127                 # the record's weights and the high digit of q2: the largest |h| there is
FRONT_RECORDS = 300


def bound_record(n_samples):
    """four hom-alt samples -- the first, both sides of the first block seam, the last -- among hom-ref ones: at 2,017 samples the entering
    record whose h h comes closest to what an i32 run can hold (16,129 a record, 1,057,030,144 over 65,536 records, below 2^30)"""
    row = np.zeros(n_samples, dtype=np.int64)
    row[[s if s < n_samples else n_samples - 1 for s in BOUND_ALT]] = 2
    row.setflags(write=False)
    return row


def _plan_case(name, n_samples, records, plan, front):
    F = random_dosage(FRONT_RECORDS, n_samples, seed=300 + n_samples) if front else None
    if F is not None:
        F.setflags(write=False)
    return dict(name=name, n_samples=n_samples, front=F, record=bound_record(n_samples), count=records - (FRONT_RECORDS if front else 0), records=records, plan=plan,
                haploid=False, maf_ppm=0, min_n=1)


def plan_cases():
    out = []
    for front in (False, True):
        tag = "_behind_random_records" if front else ""
        out.append(_plan_case("no_atomics_17_steps" + tag, BOUND_SAMPLES, 1025, [(1025, 1088, 1)], front))
        out.append(_plan_case("no_atomics_full_run_then_one_step" + tag, BOUND_SAMPLES, 65537, [(65536, 65536, 1), (1, 64, 1)], front))
        out.append(_plan_case("one_block_row_fewer_flips_to_atomics" + tag, BOUND_SAMPLES - 1, 65537, [(65537, 32832, 2)], front))
    return out


def plan_case_words(case):
    """-> uint64 [groups, 3, records]: the front's words, then the one record's `count` times"""
    one = np.repeat(M.words_from_dosage(case["record"], case["n_samples"]), case["count"], axis=2)
    if case["front"] is None:
        return np.ascontiguousarray(one)
    return np.ascontiguousarray(np.concatenate([M.words_from_dosage(case["front"], case["n_samples"]), one], axis=2))


_FRONT_SUMS = {}


def sums_in_doubles(D, n_samples):
    """M.grm_sums for a wide cohort: the model's cell weights, the two matrix products in binary64 -- exact while every sum stays below
    2^53 (asserted) -- because numpy's int64 product takes seconds at 2,017 samples"""
    X, Cc, entered = M.cell_weights(np.asarray(D, dtype=np.int64).reshape(-1, n_samples))
    assert int(np.abs(X).max(initial=0)) ** 2 * max(len(X), 1) < 2 ** 53
    a, b = M.pair_index(n_samples)
    Xf, Cf = X.astype(np.float64), Cc.astype(np.float64)
    return np.rint(Xf.T @ Xf)[a, b].astype(np.int64), np.rint(Cf.T @ Cf)[a, b].astype(np.uint64), len(X), entered


def plan_case_expected(case):
    """-> (S, N, seen, entered): the model's one-record table times the count, on top of the model's table of the front (made once per
    sample count and left unchanged)"""
    n = case["n_samples"]
    S1, N1, _, e1 = M.grm_sums(case["record"], n)
    assert e1 == 1
    S, N, entered = S1 * case["count"], N1 * np.uint64(case["count"]), case["count"]
    if case["front"] is not None:
        if n not in _FRONT_SUMS:
            _FRONT_SUMS[n] = sums_in_doubles(case["front"], n)
            for x in _FRONT_SUMS[n][:2]:
                x.setflags(write=False)
        S0, N0, _, e0 = _FRONT_SUMS[n]
        S, N, entered = S + S0, N + N0, entered + e0
    return S, N, case["records"], entered
