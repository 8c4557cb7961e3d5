"""The two plans that cut an axis into runs of whole chunks, one workgroup per run (csrc/count_plan.h): pair_count_plan cuts the words
of mg_pair_counts, sample_count_plan the records of mg_sample_counts.  The 32-bit partial sums of both kernels rest on `run <= MAX_RUN`,
which only acts above 2^27 words or 2^25 records -- out of reach of a device test -- so the header is compiled on the host by itself,
its invariants are looped over in C, and it is held against a restatement in Python and against named values.

    chunks = ceil(n / CHUNK)
    runs   = max(min(chunks, max(1, TARGET / div)), ceil(n / MAX_RUN))
    run    = ceil(chunks / runs) * CHUNK,   n_runs = ceil(n / run)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

PAIR_CHUNK, PAIR_MAX_RUN, PAIR_TARGET_WGS = 32, 1 << 20, 2048
SAMPLE_TPB, SAMPLE_MAX_RUN, SAMPLE_TARGET_WGS = 256, 1 << 20, 2048
PLANS = {"pair": (PAIR_CHUNK, PAIR_TARGET_WGS, PAIR_MAX_RUN), "sample": (SAMPLE_TPB, SAMPLE_TARGET_WGS, SAMPLE_MAX_RUN)}
DIVISORS = {"pair": (1, 2, 3, 4, 6, 8, 9, 10, 12, 16),     # the tile counts of 1..64 planes: t x t', and t (t + 1) / 2 of a square
            "sample": tuple(range(1, 65))}                 # planes
KIND = {"pair": 0, "sample": 1}
U32_MAX = (1 << 32) - 1


def plan(kind, n, div, clause=True):
    """-> (run, n_runs), the plan restated; clause False: without the MAX_RUN clause"""
    chunk, target, max_run = PLANS[kind]
    chunks = -(-n // chunk)
    runs = min(chunks, max(1, target // div))
    if clause:
        runs = max(runs, -(-n // max_run))
    run = -(-chunks // runs) * chunk
    return run, -(-n // run)


def pair_plan(n_words, tiles):
    return plan("pair", n_words, tiles)


def sample_plan(n_vars, n_planes):
    return plan("sample", n_vars, n_planes)


def pair_tiles(n_a, n_b=None):
    """the divisor mg_pair_counts hands to its plan: the tiles that compute (B NULL: those on and above the diagonal)"""
    t = lambda n: (n + 15) // 16
    return t(n_a) * (t(n_a) + 1) // 2 if n_b is None else t(n_a) * t(n_b)


def plan_np(kind, n, div):
    """the same over an array of n, in uint64"""
    chunk, target, max_run = (np.uint64(x) for x in PLANS[kind])
    one = np.uint64(1)
    n = np.asarray(n, dtype=np.uint64)
    chunks = (n + chunk - one) // chunk
    runs = np.maximum(np.minimum(chunks, np.uint64(max(1, int(target) // div))), (n + max_run - one) // max_run)
    run = (chunks + runs - one) // runs * chunk
    return run, (n + run - one) // run


def first_clause_n(kind, div):
    """the first n at which the MAX_RUN clause changes the answer: below wanted * MAX_RUN + 1 the clause asks for no more runs than
    min(chunks, wanted) already gives (n <= chunks * CHUNK <= chunks * MAX_RUN), there it asks for one more"""
    chunk, target, max_run = PLANS[kind]
    return max(1, target // div) * max_run + 1


def special_inputs(kind, div):
    ks = (1, 2, 127, 128, 129, 2047, 2048, 2049, 4095)
    n = {(k << 20) + d for k in ks for d in range(-2, 3)} | {U32_MAX} | {first_clause_n(kind, div) + d for d in range(-2, 3)}
    return np.array(sorted(x for x in n if 1 <= x <= U32_MAX), dtype=np.uint64)


SHIM = r"""
#include "count_plan.h"
typedef uint64_t (*plan_fn)(uint64_t, uint32_t, uint64_t *);
static plan_fn fn(int kind) { return kind ? mg::sample_count_plan : mg::pair_count_plan; }
extern "C" void constants(uint64_t *out)
{
    out[0] = mg::PAIR_CHUNK, out[1] = mg::PAIR_TARGET_WGS, out[2] = mg::PAIR_MAX_RUN;
    out[3] = mg::SAMPLE_TPB, out[4] = mg::SAMPLE_TARGET_WGS, out[5] = mg::SAMPLE_MAX_RUN;
}
extern "C" void plan_many(int kind, const uint64_t *n, uint64_t count, uint32_t div, uint64_t *run_out, uint64_t *n_runs_out)
{
    for (uint64_t i = 0; i < count; ++i) run_out[i] = fn(kind)(n[i], div, &n_runs_out[i]);
}
// the invariants over n[0 .. count) (n == NULL: over 1 .. count) with one divisor: 0, or the number of the invariant that fails first,
// its input in *bad
extern "C" int first_violation(int kind, const uint64_t *n, uint64_t count, uint32_t div, uint64_t *bad)
{
    const uint64_t chunk = kind ? mg::SAMPLE_TPB : mg::PAIR_CHUNK, max_run = kind ? mg::SAMPLE_MAX_RUN : mg::PAIR_MAX_RUN;
    const uint64_t target = kind ? mg::SAMPLE_TARGET_WGS : mg::PAIR_TARGET_WGS;
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t x = n ? n[i] : i + 1;
        uint64_t n_runs = 0;
        const uint64_t run = fn(kind)(x, div, &n_runs);
        const uint64_t wanted = target / div, least = (x + max_run - 1) / max_run;
        int why = 0;
        if (run % chunk != 0) why = 1;
        else if (!(chunk <= run && run <= max_run)) why = 2;
        else if (!(n_runs >= 1 && n_runs * run >= x && x > (n_runs - 1) * run)) why = 3; // (below 2^32 * 2^20: no wrap)
        else if (!(n_runs <= (wanted > least ? wanted : least))) why = 4;
        if (why) {
            *bad = x;
            return why;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """the library's own plans (csrc/count_plan.h, plain C++), compiled by themselves"""
    d = tmp_path_factory.mktemp("count_plan")
    src, so = d / "shim.cpp", d / "libcount_plan.so"
    src.write_text(SHIM)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(root, "malva_amd", "csrc"), "-o", str(so), str(src)],
                   check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    L.first_violation.restype = ctypes.c_int
    return L


def _header_plans(L, kind, n, div):
    n = np.ascontiguousarray(n, dtype=np.uint64)
    run, n_runs = np.zeros(n.size, dtype=np.uint64), np.zeros(n.size, dtype=np.uint64)
    L.plan_many(KIND[kind], n.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n.size), ctypes.c_uint32(div), run.ctypes.data_as(ctypes.c_void_p),
                n_runs.ctypes.data_as(ctypes.c_void_p))
    return run, n_runs


def test_the_constants_are_the_restatement(header):
    out = (ctypes.c_uint64 * 6)()
    header.constants(out)
    assert tuple(out) == PLANS["pair"] + PLANS["sample"]
    assert set(DIVISORS["pair"]) == {pair_tiles(a, b) for a in range(1, 65) for b in range(1, 65)} | {pair_tiles(a) for a in range(1, 65)}


@pytest.mark.parametrize("kind", ["pair", "sample"])
def test_invariants_and_the_restatement(header, kind):
    """every n in 1 .. 70,000 and the n around the multiples of 2^20, with every divisor: the invariants in C, the header equal to the
    restatement"""
    small = np.arange(1, 70_001, dtype=np.uint64)
    for div in DIVISORS[kind]:
        bad = ctypes.c_uint64(0)
        why = header.first_violation(KIND[kind], None, ctypes.c_uint64(70_000), ctypes.c_uint32(div), ctypes.byref(bad))
        assert why == 0, "invariant %d fails at n = %d, divisor %d" % (why, bad.value, div)
        special = special_inputs(kind, div)
        assert special[-1] == U32_MAX and special.size >= 9 * 5 + 1
        why = header.first_violation(KIND[kind], special.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(special.size), ctypes.c_uint32(div), ctypes.byref(bad))
        assert why == 0, "invariant %d fails at n = %d, divisor %d" % (why, bad.value, div)
        for n in (small, special):
            run, n_runs = _header_plans(header, kind, n, div)
            want_run, want_n_runs = plan_np(kind, n, div)
            differ = np.flatnonzero((run != want_run) | (n_runs != want_n_runs))
            assert differ.size == 0, "header != restatement at n = %d, divisor %d" % (int(n[differ[0]]), div)
        # the array form of the restatement is the scalar one
        for n in [int(x) for x in special] + [1, 31, 32, 33, 255, 256, 257, 4096, 4097, 8192, 8193, 65536, 65537, 70_000]:
            assert plan(kind, n, div) == tuple(int(x[0]) for x in plan_np(kind, [n], div)), (n, div)


@pytest.mark.parametrize("kind", ["pair", "sample"])
def test_the_first_n_at_which_the_clause_acts(header, kind):
    chunk, target, max_run = PLANS[kind]
    for div in DIVISORS[kind]:
        n0 = first_clause_n(kind, div)
        assert n0 <= U32_MAX
        assert plan(kind, n0, div) != plan(kind, n0, div, clause=False) and plan(kind, n0, div, clause=False)[0] == max_run + chunk
        for n in (n0 - 1, n0 - 2, n0 - chunk, n0 // 2, 1 << 20, (1 << 20) + 1, 70_000):
            assert plan(kind, n, div) == plan(kind, n, div, clause=False), (n, div)
        run, n_runs = _header_plans(header, kind, [n0 - 1, n0], div)
        assert (int(run[0]), int(n_runs[0])) == (max_run, max(1, target // div))
        assert (int(run[1]), int(n_runs[1])) == plan(kind, n0, div) and int(run[1]) < max_run and int(n_runs[1]) == max(1, target // div) + 1
    assert first_clause_n("pair", 16) == (1 << 27) + 1 and first_clause_n("sample", 64) == (1 << 25) + 1


NAMED = [
    ("pair", 16, 1_563, 32, 49),
    ("pair", 16, 4_096, 32, 128),
    ("pair", 16, 4_097, 64, 65),
    ("pair", 16, 8_193, 96, 86),
    ("pair", 10, 6_529, 64, 103),
    ("pair", 1, 65_536, 32, 2_048),
    ("pair", 1, 65_537, 64, 1_025),
    ("pair", 1, 131_073, 96, 1_366),
    ("pair", 1, 1 << 31, 1 << 20, 2_048),
    ("pair", 1, (1 << 31) + 1, 1_048_096, 2_049),
    ("pair", 16, 1 << 27, 1 << 20, 128),
    ("pair", 16, (1 << 27) + 1, 1_040_448, 129),
    ("sample", 64, 8_192, 256, 32),
    ("sample", 64, 8_193, 512, 17),
    ("sample", 64, 20_011, 768, 27),
    ("sample", 1, 524_288, 256, 2_048),
    ("sample", 1, 524_289, 512, 1_025),
    ("sample", 64, 1 << 25, 1 << 20, 32),
    ("sample", 64, (1 << 25) + 1, 1_016_832, 33),
    ("sample", 1, U32_MAX, 1 << 20, 4_096),
] + [("pair", d, U32_MAX, 1 << 20, 4_096) for d in DIVISORS["pair"]]


@pytest.mark.parametrize("kind,div,n,run,n_runs", NAMED)
def test_named_values(header, kind, div, n, run, n_runs):
    assert plan(kind, n, div) == (run, n_runs)
    got = _header_plans(header, kind, [n], div)
    assert (int(got[0][0]), int(got[1][0])) == (run, n_runs)
