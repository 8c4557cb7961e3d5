"""The host forms of the merged-batch calls share one set of device copies (stage_cells and its neighbours in malva_hip.hip): whatever a
call left there must not reach the next one.

One context goes through rounds of different sizes, the families interleaved in each, and every result is compared with what the plain
restatements of the families' own tests give for that call alone.  Every comparison is exact."""
import numpy as np
import pytest

from malva_amd import Context
from malva_amd.capi import SAMPLE_SLOTS
from test_gpu_bcf import encode_plain
from test_gpu_gp import expect_text, n_gt
from test_gpu_sample_stats import _cells_case
from test_gpu_site_tags import counts_numpy, format_masked, info_rows
from test_pairs_cpu import pack_plain, pair_plain
from test_sample_stats_cpu import sample_counts_plain

pytestmark = pytest.mark.gpu
MIN_GQ = 30
KEYS = (1, 128, 32768)
# (n_vars, planes, haploid).  The second round outgrows what the first allocated for a batch's cells (scratch keeps 25 % + 256 B of slack:
# 3 x 65 cells leave room for 307, the round has 990), and so does the fourth; the third leaves stale bytes behind the live ones -- a whole
# stale gt2 among them, which a haploid call must not read.
ROUNDS = [(65, 3, False), (330, 3, False), (40, 3, True), (65, 64, False)]


def _batch(planes, n, haploid, seed):
    """a batch's cells, drawn as tests/test_gpu_sample_stats.py draws them, with likelihoods for the GP field"""
    g1, g2, gq, vao, status, cov, cls = _cells_case(planes, n, seed)
    rng = np.random.default_rng(seed + 1)
    vgo = np.zeros(n + 1, dtype=np.uint64)
    vgo[1:] = np.cumsum([n_gt(int(a), haploid) for a in np.diff(vao.astype(np.int64))])
    probs = rng.random(size=(planes, int(vgo[-1])))
    return dict(g1=g1, g2=g2, gq=gq, vao=vao, status=status, cov=cov, cls=cls, vgo=vgo, probs=probs)


def _same_rows(got, want, what):
    assert np.array_equal(got[1], want[1]) and got[0] == want[0], what


def test_interleaved_families_over_rounds_of_different_sizes():
    rng = np.random.default_rng(7)
    table = rng.integers(0, 1 << 40, size=(64, SAMPLE_SLOTS), dtype=np.uint64)   # the tables go from round to round (the planes a round has,
    pairs = rng.integers(0, 1 << 40, size=(64, 64, 3, 3), dtype=np.uint64)       # that is; the others keep what they hold)
    with Context(35, 43, 1 << 20) as c:
        for r, (n, planes, haploid) in enumerate(ROUNDS):
            # two batches take turns, so that no call finds its own arrays where the call before it left them
            a, b = _batch(planes, n, haploid, seed=100 + r), _batch(planes, n, haploid, seed=200 + r)
            assert not np.array_equal(a["vao"], b["vao"]) and not np.array_equal(a["g1"], b["g1"])
            g2 = lambda x: None if haploid else x["g2"]
            what = "round %d (%d records, %d planes)" % (r, n, planes)

            _same_rows(c.format_calls(a["g1"], g2(a), a["gq"], haploid, a["cov"], a["vao"], min_gq=MIN_GQ),
                       format_masked(a["g1"], a["g2"], a["gq"], haploid, MIN_GQ, a["cov"], a["vao"]), what + ": format_calls")

            want_planes = pack_plain(b["g1"], b["g2"], b["gq"], haploid, b["vao"], MIN_GQ)
            assert np.array_equal(c.pack_dosage(b["g1"], g2(b), b["gq"], haploid, b["vao"], min_gq=MIN_GQ), want_planes), what + ": pack_dosage"

            got = table[:planes].copy()
            want = got + sample_counts_plain(a["g1"], a["g2"], a["gq"], haploid, a["vao"], a["status"], a["cov"], a["cls"], MIN_GQ)
            assert c.sample_counts(a["g1"], g2(a), a["gq"], haploid, a["vao"], a["status"], a["cov"], a["cls"], min_gq=MIN_GQ, counts=got) is got
            assert np.array_equal(got, want), what + ": sample_counts"
            table[:planes] = got

            ac0 = rng.integers(0, 1000, size=int(b["vao"][-1])).astype(np.uint32)
            ns0 = rng.integers(0, 1000, size=n).astype(np.uint32)
            want_ac, want_ns = counts_numpy(b["g1"], b["g2"], b["gq"], haploid, b["vao"], MIN_GQ)
            ac, ns = c.site_counts(b["g1"], g2(b), b["gq"], haploid, b["vao"], min_gq=MIN_GQ, ac=ac0.copy(), ns=ns0.copy())
            assert np.array_equal(ac, ac0 + want_ac) and np.array_equal(ns, ns0 + want_ns), what + ": site_counts"

            _same_rows(c.encode_calls_bcf(a["g1"], g2(a), a["gq"], haploid, KEYS, a["cov"], a["vao"], min_gq=MIN_GQ),
                       encode_plain(a["g1"], a["g2"], a["gq"], haploid, KEYS, a["cov"], a["vao"], MIN_GQ), what + ": encode_calls_bcf")

            got = pairs[:planes, :planes].copy()
            want = got + pair_plain(want_planes)
            assert c.pair_counts(want_planes, counts=got) is got
            assert np.array_equal(got, want), what + ": pair_counts"
            pairs[:planes, :planes] = got

            _same_rows(c.format_calls_gp(a["g1"], g2(a), a["gq"], haploid, a["vao"], a["probs"], a["vgo"], a["status"], cov=a["cov"], min_gq=MIN_GQ),
                       expect_text(a["g1"], a["g2"], a["gq"], haploid, a["vao"], a["probs"], a["vgo"], a["status"], a["cov"], MIN_GQ),
                       what + ": format_calls_gp")

            _same_rows(c.format_site_info(want_ac, want_ns, b["vao"]), info_rows(want_ac, want_ns, b["vao"]), what + ": format_site_info")
        ms = c.format_stats() + c.bcf_stats() + c.site_stats() + c.pairs_stats() + (c.sample_stats(),)
        assert len(ms) == 11 and all(np.isfinite(m) and m >= 0 for m in ms)
