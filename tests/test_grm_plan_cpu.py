"""The plan that cuts a step of mg_grm_step into pieces of records and a piece into runs, one wave per block of pairs and run
(csrc/grm_plan.h).  The i32 accumulators of grm_gram_kernel rest on `run <= GRM_MAX_RUN`, and the form without atomics on `runs == 1`;
most of the plan's range -- 16,384 samples, 2^32 - 1 records, a cap of 4,096 MiB -- is out of reach of a device test, so the header is
compiled on the host by itself, its invariants are looped over in C, and it is held against a restatement in Python and against named
values.

    rows      = ceil(n_samples / BLOCK) * BLOCK,   blocks = rows / BLOCK,   upper = blocks (blocks + 1) / 2
    piece_max = max(K, floor(cap / (3 rows) / K) * K);   the pieces: piece_max, piece_max, ..., what is left
    ld        = ceil(piece / K) * K,   steps = ld / K
    runs      = min(max(ceil(ld / MAX_RUN), min(ceil(FILL / upper), ceil(ld / MIN_RUN))), steps, 65535)
    run       = ceil(steps / runs) * K,   n_runs = ceil(ld / run)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

GRM_K, GRM_BLOCK, GRM_MAX_RUN, GRM_FILL, GRM_MIN_RUN = 64, 32, 65536, 2048, 1024
MAX_SAMPLES, U32_MAX = 16384, (1 << 32) - 1
SCRATCH_MB = (1, 384, 4096)


def grm_rows(n_samples):
    return -(-n_samples // GRM_BLOCK) * GRM_BLOCK


def piece_max(rows, scratch_mb):
    return max(GRM_K, (scratch_mb << 20) // (3 * rows) // GRM_K * GRM_K)


def run_plan(ld, blocks, max_run=GRM_MAX_RUN):
    """-> (run, n_runs) of a piece whose padded row is ld"""
    upper = blocks * (blocks + 1) // 2
    steps = ld // GRM_K
    runs = max(-(-ld // max_run), min(-(-GRM_FILL // upper), -(-ld // GRM_MIN_RUN)))
    runs = min(runs, steps, 65535)
    run = -(-steps // runs) * GRM_K
    return run, -(-ld // run)


def step_plan(n_samples, n_vars, scratch_mb=384, max_run=GRM_MAX_RUN):
    """-> [(piece, run, n_runs)]: the pieces of one step in their order, with the run and the runs of each; n_runs == 1 is the Gram kernel
    without atomics"""
    rows = grm_rows(n_samples)
    pm = piece_max(rows, scratch_mb)
    out = []
    for v0 in range(0, n_vars, pm):
        piece = min(pm, n_vars - v0)
        out.append((piece,) + run_plan(-(-piece // GRM_K) * GRM_K, rows // GRM_BLOCK, max_run))
    return out


def record_counts():
    """the record counts around every multiple of 64 up to 4,160, of 1,024 up to 140,288 and of 65,536 (1 .. 16 times, then 2^k times up to
    2^31), and the last ones a call takes"""
    n = {64 * k + d for k in range(1, 66) for d in (-1, 0, 1)} | {1024 * k + d for k in range(1, 138) for d in (-1, 0, 1)}
    n |= {65536 * k + d for k in list(range(1, 17)) + [1 << e for e in range(5, 16)] for d in (-1, 0, 1)} | {1, 2, U32_MAX - 1, U32_MAX}
    return np.array(sorted(x for x in n if 1 <= x <= U32_MAX), dtype=np.uint64)


SHIM = r"""
#include "grm_plan.h"
extern "C" void constants(uint64_t *out)
{
    out[0] = mg::GRM_K, out[1] = mg::GRM_BLOCK, out[2] = mg::GRM_MAX_RUN, out[3] = mg::GRM_FILL, out[4] = mg::GRM_MIN_RUN;
}
// the step of n_vars records cut as mg_grm_step_device cuts it: out[4 i ..] = piece, ld, run, n_runs of piece i -> the number of pieces
// (at most max_pieces are written)
extern "C" uint64_t step_plan(uint32_t n_samples, uint64_t n_vars, uint32_t scratch_mb, uint64_t *out, uint64_t max_pieces)
{
    const uint32_t rows = mg::grm_rows(n_samples), blocks = rows / mg::GRM_BLOCK;
    const uint64_t piece_max = mg::grm_piece_max(rows, (uint64_t)scratch_mb << 20);
    uint64_t k = 0;
    for (uint64_t v0 = 0; v0 < n_vars; v0 += piece_max, ++k) {
        const uint64_t piece = piece_max < n_vars - v0 ? piece_max : n_vars - v0;
        if (k < max_pieces) {
            out[4 * k] = piece, out[4 * k + 1] = mg::grm_ld(piece);
            out[4 * k + 2] = mg::grm_run_plan(out[4 * k + 1], blocks, &out[4 * k + 3]);
        }
    }
    return k;
}
static int piece_violation(uint64_t piece, uint32_t rows, uint64_t cap)
{
    const uint32_t blocks = rows / mg::GRM_BLOCK;
    const uint64_t ld = mg::grm_ld(piece), upper = (uint64_t)blocks * (blocks + 1) / 2;
    uint64_t runs = 0;
    const uint64_t run = mg::grm_run_plan(ld, blocks, &runs);
    if (!(ld % mg::GRM_K == 0 && ld >= piece && ld - piece < mg::GRM_K)) return 7;
    if (run % mg::GRM_K != 0) return 1;
    if (!(mg::GRM_K <= run && run <= mg::GRM_MAX_RUN)) return 2;
    if (!(runs >= 1 && runs * run >= ld && ld > (runs - 1) * run)) return 3;
    if (!(runs <= 65535)) return 4;
    if (!(3ull * rows * ld <= cap || ld == mg::GRM_K)) return 6;
    // one run, the form without atomics, exactly where the piece is short or the blocks alone fill the device
    if ((runs == 1) != (ld <= mg::GRM_MIN_RUN || (upper >= mg::GRM_FILL && ld <= mg::GRM_MAX_RUN))) return 8;
    return 0;
}
// the invariants over samples 1 .. max_samples, the record counts n[0 .. count) and the caps mb[0 .. n_mb): 0, or the number of the
// invariant that fails first, its input in bad[0 .. 3)
extern "C" int first_violation(uint32_t max_samples, const uint64_t *n, uint64_t count, const uint32_t *mb, uint32_t n_mb, uint64_t *bad)
{
    for (uint32_t s = 1; s <= max_samples; ++s) {
        const uint32_t rows = mg::grm_rows(s);
        for (uint32_t m = 0; m < n_mb; ++m) {
            const uint64_t cap = (uint64_t)mb[m] << 20, piece_max = mg::grm_piece_max(rows, cap);
            int why = 0;
            if (!(rows % mg::GRM_BLOCK == 0 && rows >= s && rows - s < mg::GRM_BLOCK)) why = 9;
            else if (!(piece_max % mg::GRM_K == 0 && piece_max >= mg::GRM_K)) why = 10;
            for (uint64_t i = 0; i < count && !why; ++i) {
                // the pieces: piece_max each but the last, which is what is left -- they cover n_vars exactly
                const uint64_t pieces = (n[i] + piece_max - 1) / piece_max, last = n[i] - (pieces - 1) * piece_max;
                if (!(pieces >= 1 && last >= 1 && last <= piece_max && (pieces - 1) * piece_max + last == n[i])) why = 5;
                if (!why && pieces > 1) why = piece_violation(piece_max, rows, cap);
                if (!why) why = piece_violation(last, rows, cap);
                if (why) bad[1] = n[i];
            }
            if (why) {
                bad[0] = s, bad[2] = mb[m];
                return why;
            }
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """the library's own plan (csrc/grm_plan.h, plain C++), compiled by itself"""
    d = tmp_path_factory.mktemp("grm_plan")
    src, so = d / "shim.cpp", d / "libgrm_plan.so"
    src.write_text(SHIM)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(root, "malva_amd", "csrc"), "-o", str(so), str(src)],
                   check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    L.first_violation.restype = ctypes.c_int
    L.step_plan.restype = ctypes.c_uint64
    return L


def _header_step(L, n_samples, n_vars, scratch_mb=384, max_pieces=64):
    out = np.zeros(4 * max_pieces, dtype=np.uint64)
    k = L.step_plan(ctypes.c_uint32(n_samples), ctypes.c_uint64(n_vars), ctypes.c_uint32(scratch_mb), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(max_pieces))
    rows = out[:4 * min(k, max_pieces)].reshape(-1, 4)
    return k, [(int(r[0]), int(r[2]), int(r[3])) for r in rows]


def test_the_constants_are_the_restatement(header):
    out = (ctypes.c_uint64 * 5)()
    header.constants(out)
    assert tuple(out) == (GRM_K, GRM_BLOCK, GRM_MAX_RUN, GRM_FILL, GRM_MIN_RUN)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "malva_amd", "csrc", "malva_hip.hip")).read()
    assert "grm_run_plan(" in src and "grm_piece_max(" in src and '#include "grm_plan.h"' in src, "the library cuts its steps by this header"


def test_invariants_over_every_sample_count(header):
    """samples 1 .. 16,384, the record counts of record_counts(), caps of 1, 384 and 4,096 MiB: a run is whole MFMA steps, between GRM_K and
    GRM_MAX_RUN, the runs cover the padded row and none is empty, there are at most 65,535, the pieces cover the step exactly, a piece's
    byte images fit the cap unless it is one MFMA step, and one run is made exactly where the issue of atomics says"""
    n = record_counts()
    assert n.size > 600 and int(n[-1]) == U32_MAX
    mb = np.array(SCRATCH_MB, dtype=np.uint32)
    bad = (ctypes.c_uint64 * 3)()
    why = header.first_violation(ctypes.c_uint32(MAX_SAMPLES), n.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n.size), mb.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.c_uint32(mb.size), bad)
    assert why == 0, "invariant %d fails at %d samples, %d records, %d MiB" % (why, bad[0], bad[1], bad[2])


def test_the_header_is_the_restatement(header):
    """block counts all along the range (the sample counts on both sides of a block), record counts up to 2^24, the three caps"""
    samples = sorted({s for b in range(1, MAX_SAMPLES // GRM_BLOCK + 1, 41) for s in (GRM_BLOCK * b - 31, GRM_BLOCK * b)} | {1, 33, 508, 509, 2016, 2017, MAX_SAMPLES})
    counts = [int(x) for x in record_counts() if x <= 1 << 24][::11] + [1024, 1025, 65536, 65537, 140000]
    for mb in SCRATCH_MB:
        for s in samples:
            for n in counts:
                want = step_plan(s, n, mb)
                if len(want) > 64:
                    continue
                k, got = _header_step(header, s, n, mb)
                assert (k, got) == (len(want), want), (s, n, mb)


# (samples, records, MiB) -> the pieces as (records, run, runs)
NAMED = [
    ((508, 140_000, 384), [(140_000, 8_768, 16)]),
    ((2_016, 65_537, 384), [(65_537, 32_832, 2)]),
    ((2_017, 65_537, 384), [(65_536, 65_536, 1), (1, 64, 1)]),
    ((2_017, 65_536, 384), [(65_536, 65_536, 1)]),
    ((2_017, 1_025, 384), [(1_025, 1_088, 1)]),
    ((2_016, 1_025, 384), [(1_025, 576, 2)]),
    ((33, 1_024, 384), [(1_024, 1_024, 1)]),
    ((33, 1_025, 384), [(1_025, 576, 2)]),
    ((140, 4_200, 1), [(2_176, 768, 3), (2_024, 1_024, 2)]),
    ((16_384, 1, 1), [(1, 64, 1)]),
    ((16_384, 129, 1), [(64, 64, 1), (64, 64, 1), (1, 64, 1)]),
    ((16_384, 65_537, 4_096), [(65_537, 32_832, 2)]),
]


@pytest.mark.parametrize("key,pieces", NAMED, ids=["%d-%d-%d" % k for k, _ in NAMED])
def test_named_values(header, key, pieces):
    assert step_plan(*key) == pieces
    assert _header_step(header, *key) == (len(pieces), pieces)


def test_the_ends_of_the_range(header):
    """2^32 - 1 records of 16,384 samples under a cap of 4,096 MiB: 87,381 records a piece ... and under 1 MiB one MFMA step a piece"""
    k, first = _header_step(header, MAX_SAMPLES, U32_MAX, 4096, max_pieces=1)
    pm = piece_max(MAX_SAMPLES, 4096)
    assert pm == 87_360 and k == -(-U32_MAX // pm) and first == [(pm, 43_712, 2)]
    k, first = _header_step(header, MAX_SAMPLES, U32_MAX, 1, max_pieces=1)
    assert piece_max(MAX_SAMPLES, 1) == GRM_K and k == -(-U32_MAX // GRM_K) and first == [(64, 64, 1)]
    # the longest piece there is: 32 samples or fewer under 4,096 MiB, and the most runs any piece takes
    pm = piece_max(GRM_BLOCK, 4096)
    run, runs = run_plan(pm, 1)
    assert pm == 44_739_200 and (run, runs) == (21_888, 2_045) and run <= GRM_MAX_RUN
    assert _header_step(header, 1, pm, 4096) == (1, [(pm, run, runs)])
