"""`call --cohort --ld PATH`: r2 between nearby records along the samples -- the records' words over the samples
(mg_pack_site_dosage) and the pairs of a window (mg_ld_window), both made on the device.

The ABI is compared with the restatement of tests/ld_model.py; the command line with that restatement applied to the merged VCF the
same run wrote.  Every comparison is exact: the counts are integers, and r2 is compared bit for bit (two correctly rounded conversions
and one division)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ld_cases
from ld_model import LD_PAIR, ld_candidates, ld_filter, ld_pairs, ld_table_text, site_words
from malva_amd import Context, MalvaError, capi

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE, MG_ERR_LIMIT = -1, -3, -5
MIN_GQ = 30
POISON = 0xDEADBEEFDEADBEEF
PAD = 8


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def _dev(a):
    """a host array -> a device tensor of its bytes (at least one element)"""
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1) if a.size else np.zeros(8, dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(torch.device("cuda", 0))


def _same(got, want):
    """two LD_PAIR arrays, field by field, r2 by its bits"""
    assert got.dtype == LD_PAIR and len(got) == len(want)
    for f in ("i", "j", "n", "sign"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["r2"].view(np.uint64), want["r2"].view(np.uint64)), "r2 differs in its bits"


# ---- the ABI: the pack ---------------------------------------------------------------------------------------------------------------

def _cells_case(planes, n, seed):
    """records of 1, 2 and 3 alleles in turn (the turn starts where `planes` says), allele indexes -1 .. A inclusive (mostly inside), GQ
    on both sides of MIN_GQ"""
    rng = np.random.default_rng(seed)
    A = np.array([(1, 2, 2, 3)[(v + planes) % 4] for v in range(n)], dtype=np.int64)
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)

    def draw():
        g = (rng.random((planes, n)) * A[None, :]).astype(np.int64)
        stray = rng.random((planes, n)) < 0.1
        g[stray] = np.where(rng.random(int(stray.sum())) < 0.5, -1, np.broadcast_to(A[None, :], (planes, n))[stray])
        return g.astype(np.int32)
    g1, g2 = draw(), draw()
    gq = rng.integers(MIN_GQ - 20, MIN_GQ + 20, size=(planes, n)).astype(np.int32)
    if n:
        gq[0, 0], gq[planes - 1, n - 1] = MIN_GQ, MIN_GQ - 1
    return g1, g2, gq, vao


@pytest.fixture(scope="module")
def cells():
    made = {}

    def get(planes, n):
        if (planes, n) not in made:
            made[(planes, n)] = _cells_case(planes, n, seed=planes * 1000 + n)
            for x in made[(planes, n)]:
                x.setflags(write=False)
        return made[(planes, n)]
    return get


def _transpose(planes_words, n):
    """mg_pack_dosage's [planes, 3, W] -> [3, n]: bit p of [d, v] = bit v & 63 of word v >> 6 of [p, d]"""
    P = planes_words.shape[0]
    out = np.zeros((3, n), dtype=np.uint64)
    v = np.arange(n)
    for p in range(P):
        for d in range(3):
            bit = (planes_words[p, d][v >> 6] >> (v & 63).astype(np.uint64)) & np.uint64(1) if n else np.zeros(0, dtype=np.uint64)
            out[d] |= bit << np.uint64(p)
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("haploid", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("planes", [1, 2, 63, 64])
def test_pack_equals_the_model(ctx, cells, planes, n, haploid, masked):
    g1, g2, gq, vao = cells(planes, n)
    q = MIN_GQ if masked else None
    want = site_words(g1, g2, gq, haploid, vao, q)
    if n >= 63 and planes >= 2:
        assert all(want[d].any() for d in ((0, 2) if haploid else (0, 1, 2))) and not want[:, np.diff(vao.astype(np.int64)) != 2].any()
    if planes < 64:
        assert not (want >> np.uint64(planes)).any()
    got = ctx.pack_site_dosage(g1, None if haploid else g2, gq if masked else None, haploid, vao, min_gq=q)
    assert np.array_equal(got, want), "host form"
    # the bit-transpose of mg_pack_dosage's planes over the same cells
    assert np.array_equal(_transpose(ctx.pack_dosage(g1, None if haploid else g2, gq if masked else None, haploid, vao, min_gq=q), n), want)
    # the device form into a poisoned buffer between guard words: every word is written, nothing beyond
    d1, d2, dq, dv = _dev(g1), _dev(g2), _dev(gq), _dev(vao)
    out = _dev(np.full(3 * n + 2 * PAD, POISON, dtype=np.uint64))
    torch.cuda.synchronize()
    ctx.pack_site_dosage_device(n, planes, haploid, d1.data_ptr(), 0 if haploid else d2.data_ptr(), dq.data_ptr() if masked else 0, dv.data_ptr(),
                                out.data_ptr() + 8 * PAD, min_gq=q)
    ctx.synchronize()
    h = out.cpu().numpy().view(np.uint64)
    assert (h[:PAD] == POISON).all() and (h[PAD + 3 * n:] == POISON).all(), "written outside the words"
    assert np.array_equal(h[PAD:PAD + 3 * n].reshape(3, n), want), "device form"


def test_pack_argument_errors(ctx, cells):
    g1, g2, gq, vao = cells(2, 65)
    L, h = ctx._L, ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros((3, 65), dtype=np.uint64)
    for form in (L.mg_pack_site_dosage, L.mg_pack_site_dosage_device):
        assert form(h, 65, 0, 0, p(g1), p(g2), p(gq), 0, 0, p(vao), p(out)) == MG_ERR_ARG
        assert form(h, 65, 65, 0, p(g1), p(g2), p(gq), 0, 0, p(vao), p(out)) == MG_ERR_ARG
        assert form(h, 65, 2, 0, None, p(g2), p(gq), 0, 0, p(vao), p(out)) == MG_ERR_ARG
        assert form(h, 65, 2, 0, p(g1), None, p(gq), 0, 0, p(vao), p(out)) == MG_ERR_ARG
        assert form(h, 65, 2, 0, p(g1), p(g2), None, 1, MIN_GQ, p(vao), p(out)) == MG_ERR_ARG
        assert form(h, 65, 2, 0, p(g1), p(g2), p(gq), 0, 0, None, p(out)) == MG_ERR_ARG
        assert form(h, 65, 2, 0, p(g1), p(g2), p(gq), 0, 0, p(vao), None) == MG_ERR_ARG
        assert form(None, 65, 2, 0, p(g1), p(g2), p(gq), 0, 0, p(vao), p(out)) == MG_ERR_ARG
    assert not out.any()
    assert L.mg_pack_site_dosage(h, 0, 2, 1, None, None, None, 0, 0, p(vao), None) == 0      # no records: nothing to write


# ---- the ABI: the window -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tables():
    """the random tables of ld_cases.window_case with their candidates (every pair of the window with an r2), made once and left unchanged"""
    made = {}

    def get(window, n_vars, n_groups):
        key = (window, n_vars, n_groups)
        if key not in made:
            words, chrom, pos, max_bp = ld_cases.window_case(window, n_vars, n_groups)
            cand = ld_candidates(words, window)
            cand.setflags(write=False)
            made[key] = (words, chrom, pos, max_bp, cand)
        return made[key]
    return get


def _device_window(ctx, words, chrom, pos, n_first, window, max_bp, min_n, min_r2, cap):
    """the device form into poisoned buffers between guard words -> (rc, needed, pairs [cap], row_off)"""
    G, _, n = words.shape
    ds, dc, dp = _dev(words), _dev(chrom), _dev(pos)
    pairs = _dev(np.full(3 * (cap + 2 * PAD), POISON, dtype=np.uint64))
    off = _dev(np.full(n_first + 1 + 2 * PAD, POISON, dtype=np.uint64))
    torch.cuda.synchronize()
    rc, need = ctx.ld_window_device(n, n_first, G, ds.data_ptr(), dc.data_ptr(), dp.data_ptr(), window, max_bp, min_n, min_r2,
                                    pairs.data_ptr() + 24 * PAD if cap else 0, cap, off.data_ptr() + 8 * PAD)
    ctx.synchronize()
    hp, ho = pairs.cpu().numpy().view(np.uint64), off.cpu().numpy().view(np.uint64)
    assert (hp[:3 * PAD] == POISON).all() and (hp[3 * (PAD + cap):] == POISON).all(), "written outside the pairs' buffer"
    assert (ho[:PAD] == POISON).all() and (ho[PAD + n_first + 1:] == POISON).all(), "written outside row_off"
    return rc, need, hp[3 * PAD:3 * (PAD + cap)].copy().view(LD_PAIR), ho[PAD:PAD + n_first + 1].copy()


def _check(ctx, words, chrom, pos, cand, n_first, window, max_bp, min_n, min_r2, caps=False):
    want, want_off = ld_filter(cand, chrom, pos, n_first, max_bp, min_n, min_r2)
    got, off = ctx.ld_window(words, chrom, pos, window, n_first=n_first, max_bp=max_bp, min_n=min_n, min_r2=min_r2)
    _same(got, want)
    assert np.array_equal(off, want_off)
    if not caps:
        return want
    k = len(want)
    rc, need, pairs, off = _device_window(ctx, words, chrom, pos, n_first, window, max_bp, min_n, min_r2, k)       # the buffer exact
    assert (rc, need) == (0, k) and np.array_equal(off, want_off)
    _same(pairs, want)
    for cap in sorted({max(k - 1, 0), 0}):                                                                           # one less, and none
        if cap == k:
            continue
        rc, need, pairs, off = _device_window(ctx, words, chrom, pos, n_first, window, max_bp, min_n, min_r2, cap)
        assert (rc, need) == (MG_ERR_LIMIT, k) and np.array_equal(off, want_off), "the count and row_off are right all the same"
        _same(pairs, want[:cap])
        with pytest.raises(MalvaError) as e:                                                                         # the host form
            ctx.ld_window(words, chrom, pos, window, n_first=n_first, max_bp=max_bp, min_n=min_n, min_r2=min_r2, pairs_cap=cap)
        assert e.value.code == MG_ERR_LIMIT and e.value.needed == k and np.array_equal(e.value.row_off, want_off)
        _same(e.value.pairs[:cap], want[:cap])
        assert not e.value.pairs[cap:].view(np.uint8).any(), "written at or behind pairs_cap"
    return want


@pytest.mark.parametrize("n_groups", ld_cases.GROUPS)
@pytest.mark.parametrize("window,n_vars", [(w, n) for w in ld_cases.WINDOWS for n in ld_cases.n_vars_for(w)])
def test_window_equals_the_model(ctx, tables, window, n_vars, n_groups):
    words, chrom, pos, max_bp, cand = tables(window, n_vars, n_groups)
    n = n_vars
    above = 64 * n_groups + 1                                                       # more samples than the cohort has
    main = _check(ctx, words, chrom, pos, cand, n, window, 0, 1, 0.2, caps=True)
    every = _check(ctx, words, chrom, pos, cand, n, window, 0, 1, 0.0)
    assert len(every) >= len(main)
    for n_first in sorted({0, min(1, n), max(n - window, 0)}):
        _check(ctx, words, chrom, pos, cand, n_first, window, max_bp, 1, 0.2, caps=n_first == 1)
    _check(ctx, words, chrom, pos, cand, n, window, max_bp, 2, 0.0)
    _check(ctx, words, chrom, pos, cand, n, window, 0, 1, 1.0)
    assert len(_check(ctx, words, chrom, pos, cand, n, window, 0, above, 0.0)) == 0
    # the table walked in chunks with a look-ahead of `window` records equals the table in one call
    step = max(1, n // 3)
    parts = []
    for c0 in range(0, n, step):
        c1 = min(n, c0 + step + window)
        part, off = ctx.ld_window(words[:, :, c0:c1], chrom[c0:c1], pos[c0:c1], window, n_first=min(step, n - c0), max_bp=max_bp, min_n=1, min_r2=0.2)
        part = part.copy()
        part["i"] += c0
        part["j"] += c0
        parts.append(part)
    whole, _ = ld_filter(cand, chrom, pos, n, max_bp, 1, 0.2)
    _same(np.concatenate(parts) if parts else np.zeros(0, dtype=LD_PAIR), whole)


def test_window_over_a_ragged_last_chunk_of_groups(ctx):
    """17 groups: one more than the kernel stages at a time"""
    words, chrom, pos, max_bp = ld_cases.window_case(64, 130, 17)
    cand = ld_candidates(words, 64)
    assert len(_check(ctx, words, chrom, pos, cand, 130, 64, 0, 1, 0.2, caps=True)) > 100
    _check(ctx, words, chrom, pos, cand, 100, 64, max_bp, 3, 0.0)


CASES = ld_cases.directed_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_window_on_a_directed_case(ctx, case):
    p = case["params"]
    want, want_off = ld_pairs(case["words"], case["chrom"], case["pos"], **p)
    got, off = ctx.ld_window(case["words"], case["chrom"], case["pos"], p["window"], n_first=p["n_first"], max_bp=p["max_bp"], min_n=p["min_n"], min_r2=p["min_r2"])
    _same(got, want)
    assert np.array_equal(off, want_off)
    here = [(int(x["i"]), int(x["j"])) for x in got]
    assert (case["pair"] in here) == (case["says"] == "emitted")
    if case["sign"] is not None and case["says"] == "emitted":
        assert int(got[here.index(case["pair"])]["sign"]) == case["sign"]


def test_window_argument_errors(ctx):
    words, chrom, pos, _ = ld_cases.window_case(3, 5, 2)
    L, h = ctx._L, ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pairs, off, need = np.zeros(64, dtype=LD_PAIR), np.zeros(6, dtype=np.uint64), C.c_uint64(77)
    ok = dict(n_vars=5, n_first=5, n_groups=2, sites=p(words), chrom=p(chrom), pos=p(pos), window=3, max_bp=0, min_n=1, min_r2=0.2, pairs=p(pairs), cap=64, off=p(off),
              need=C.byref(need))
    bad = [dict(n_groups=0), dict(n_groups=capi.LD_MAX_GROUPS + 1), dict(window=0), dict(window=capi.LD_MAX_WINDOW + 1), dict(min_r2=-0.1), dict(min_r2=1.5),
           dict(min_r2=float("nan")), dict(min_r2=float("inf")), dict(min_n=0), dict(n_first=6), dict(sites=None), dict(chrom=None), dict(pos=None), dict(off=None),
           dict(need=None), dict(pairs=None)]
    for form in (L.mg_ld_window, L.mg_ld_window_device):
        for change in bad:
            a = dict(ok, **change)
            assert form(h, *a.values()) == MG_ERR_ARG, change
        assert form(None, *ok.values()) == MG_ERR_ARG
    assert not pairs.view(np.uint8).any() and not off.any() and need.value == 77, "an argument error writes nothing"
    assert L.mg_ld_window(h, *ok.values()) == 0 and need.value == int(off[5])
    empty = dict(ok, n_vars=0, n_first=0, sites=None, chrom=None, pos=None, pairs=None, cap=0)      # no records: legal, row_off[0] = 0
    off[:] = 9
    assert L.mg_ld_window(h, *empty.values()) == 0 and need.value == 0 and off[0] == 0 and (off[1:] == 9).all()
    assert L.mg_ld_stats(h, None) == MG_ERR_ARG


def test_ld_stats_before_and_after():
    with Context(35, 43, 1 << 20) as c:
        ms = (C.c_float * 2)(5.0, 5.0)
        assert c._L.mg_ld_stats(c.h, ms) == MG_ERR_STATE
        with pytest.raises(MalvaError) as e:
            c.ld_stats()
        assert e.value.code == MG_ERR_STATE
        words, chrom, pos, _ = ld_cases.window_case(3, 69, 2)
        c.ld_window(words, chrom, pos, 3)
        ms = c.ld_stats()
        assert ms[0] == 0 and ms[1] > 0, "the pack was not called yet"
        c.pack_site_dosage(np.zeros((2, 0), dtype=np.int32), None, None, True, np.zeros(1, dtype=np.uint32))
        after = c.ld_stats()                                                        # no records: the call still counts as one
        assert after[0] >= 0 and after[1] == ms[1]


def test_the_ld_calls_and_their_neighbours_do_not_disturb_each_other(cells):
    """one context: the neighbours, the two calls, the neighbours again -- every result what it is alone; a call of one kind leaves the
    timers of the others what they were"""
    g1, g2, gq, vao = cells(63, 257)
    words, chrom, pos, max_bp = ld_cases.window_case(64, 130, 3)
    want_words = site_words(g1, g2, gq, False, vao, MIN_GQ)
    want, want_off = ld_pairs(words, chrom, pos, 130, 64, max_bp, 1, 0.2)
    with Context(35, 43, 1 << 20) as c:
        def neighbours():
            planes = c.pack_dosage(g1, g2, gq, False, vao, min_gq=MIN_GQ)
            counts = c.pair_counts(planes)
            n, het, hom = c.site_geno_counts(g1, g2, gq, False, vao, min_gq=MIN_GQ)
            return (planes.tobytes(), counts.tobytes(), n.tobytes(), het.tobytes(), hom.tobytes()), c.pairs_stats() + c.hwe_stats()
        res0, _ = neighbours()
        before = c.pairs_stats() + c.hwe_stats()
        got_words = c.pack_site_dosage(g1, g2, gq, False, vao, min_gq=MIN_GQ)
        ms_pack = c.ld_stats()
        got, off = c.ld_window(words, chrom, pos, 64, max_bp=max_bp, min_r2=0.2)
        assert c.pairs_stats() + c.hwe_stats() == before, "the LD calls changed a neighbour's timer"
        ms = c.ld_stats()
        assert ms[0] == ms_pack[0], "mg_ld_window changed the timer of mg_pack_site_dosage"
        res1, _ = neighbours()
        assert res1 == res0 and c.ld_stats() == ms, "a neighbour changed mg_ld_stats"
        again_words = c.pack_site_dosage(g1, g2, gq, False, vao, min_gq=MIN_GQ)
        again, off2 = c.ld_window(words, chrom, pos, 64, max_bp=max_bp, min_r2=0.2)
        assert np.array_equal(got_words, want_words) and np.array_equal(again_words, want_words)
        _same(got, want)
        _same(again, want)
        assert np.array_equal(off, want_off) and np.array_equal(off2, want_off)


# ---- the command line -------------------------------------------------------------------------------------------------------------

from test_gpu_merged import BIN, COMMON, _cli, _no_leftovers, _split, haploid_cohort  # noqa: E402,F401 (the fixture)
from test_gpu_site_tags import _median_gq  # noqa: E402
from ld_model import HEADER  # noqa: E402


def _lines(table):
    lines = table.split("\n")
    assert lines[-1] == "" and lines[0] + "\n" == HEADER
    return [l.split("\t") for l in lines[1:-1]]


def _check_ld_cohort(run, groups, tmp_path, ld_opts, model_opts):
    """run(opts, group, directory, env, table) writes directory/m.vcf and, if table, directory/ld.tsv; groups: the grouped runs that must
    give the same bytes.  The expected table is the model applied to the merged VCF the same run wrote."""
    tables = {}
    q = None
    for tag in ("all", "masked"):
        opts = ld_opts + ([] if q is None else ["--min-gq", str(q)])
        d = tmp_path / tag
        d.mkdir()
        run(opts, [], d, {}, True)
        _no_leftovers(d, ["m.vcf", "ld.tsv"])
        merged = open(str(d / "m.vcf")).read()
        table = open(str(d / "ld.tsv")).read()
        assert table == ld_table_text(merged, min_gq=q, **model_opts), tag
        tables[tag] = table
        for i, (group, batch) in enumerate(groups):                                # whatever the grouping, the batches and the chunks: the same bytes
            g = tmp_path / ("%s-g%d" % (tag, i))
            g.mkdir()
            run(opts, group, g, {"MALVA_GENO_BATCH": batch}, True)
            _no_leftovers(g, ["m.vcf", "ld.tsv"])
            assert open(str(g / "ld.tsv")).read() == table, "%s %s batch %s" % (tag, group, batch)
            assert open(str(g / "m.vcf")).read() == merged
        if q is None:
            plain = tmp_path / "plain"                                             # without --ld: the same merged file
            plain.mkdir()
            run([], [], plain, {}, False)
            _no_leftovers(plain, ["m.vcf"])
            assert open(str(plain / "m.vcf")).read() == merged
            q = _median_gq(merged)
    assert tables["all"] != tables["masked"], "--min-gq %d changes nothing in the table" % q
    return tables


def test_cli_ld_on_the_haploid_cohort(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    _cli(["index"] + COMMON + [fa, vcf, fq])

    def run(opts, group, d, env, table):
        assert _cli(["call"] + COMMON + opts + group + ["--cohort", "--merged", str(d / "m.vcf")] + (["--ld", str(d / "ld.tsv")] if table else []) + [fa, vcf, man],
                    env=dict(os.environ, **env)) == ""
    # windows of 5 records in batches and chunks of 3 and 7: they cross both
    tables = _check_ld_cohort(run, [(["--cohort-group", "2"], "3"), (["--cohort-group", "3"], "7"), ([], "3")], tmp_path,
                              ["--ld-window", "5", "--ld-min-r2", "0"], dict(window=5, min_r2=0.0))
    rows = _lines(tables["all"])
    assert len(rows) > 20 and {r[7] for r in rows} >= {"+", "-"} and all(2 <= int(r[5]) <= 4 for r in rows)
    assert any(r[6] == "1" for r in rows) and any(r[6] not in ("0", "1") for r in rows)
    # the defaults (window 64, 1 Mb, r2 >= 0.2, n >= 2), and -o alone, without --merged: one group, and groups of 3 + 1
    merged = open(str(tmp_path / "all" / "m.vcf")).read()
    want = ld_table_text(merged)
    assert 1 < len(_lines(want)) < len(rows) * 20
    for i, group in enumerate(([], ["--cohort-group", "3"])):
        d = tmp_path / ("o%d" % i)
        d.mkdir()
        assert _cli(["call"] + COMMON + group + ["--cohort", "-o", str(d / "out"), "--ld", str(d / "ld.tsv"), fa, vcf, man]) == ""
        _no_leftovers(d, ["out", "ld.tsv"])
        assert open(str(d / "ld.tsv")).read() == want
    # every sub-option at once
    d = tmp_path / "opts"
    d.mkdir()
    assert _cli(["call"] + COMMON + ["--cohort", "--merged", str(d / "m.vcf"), "--ld", str(d / "ld.tsv"), "--ld-window", "3", "--ld-window-bp", "2000", "--ld-min-r2", "0.5",
                                     "--ld-min-n", "4", fa, vcf, man]) == ""
    got = open(str(d / "ld.tsv")).read()
    assert got == ld_table_text(merged, window=3, max_bp=2000, min_r2=0.5, min_n=4) and all(r[5] == "4" for r in _lines(got))
    _no_leftovers(tmp, ["haploid.fq", "dump.txt", "sim1.fq", "sim2.fq", "keep.txt", "cohort.tsv"] + [f for f in os.listdir(tmp) if f.startswith("haploid.vcf.gz")])


def test_cli_ld_on_general_blocks(tmp_path):
    """the diploid panel of tests/test_gpu_merged.py::test_cli_merged_on_general_blocks: multi-allelic records (partners that give no pair)
    and heterozygous cells; grouped runs in batches and chunks of 7 records under windows of 64"""
    from malva_amd import synth
    from test_gpu_cohort import _sample_table
    data = tmp_path / "data"
    data.mkdir()
    panel = synth.indel_panel(1_500, seed=21, n_samples=70)
    prefix = str(data / "p")
    synth.write_vcf_fasta(panel, prefix)
    k, ref_k = 35, 43
    names = []
    for s in range(3):
        hi, lo, cnt = _sample_table(synth.flat_kmer_table(panel, 60_000, k, ref_k, seed=5, max_records=1_200), s)
        rows = synth.unpack_ascii(hi, lo, ref_k)
        with open(str(data / ("s%d.txt" % s)), "w") as fh:
            for r, c in zip(rows, cnt):
                fh.write("%s\t%d\n" % (bytes(r[:ref_k]).decode(), int(c)))
        names.append("s%d" % s)
    (data / "cohort.tsv").write_text("".join("%s\t%s\n" % (n, n) for n in names))
    common = ["-k", str(k), "-r", str(ref_k), "-b", "1", prefix + ".fa", prefix + ".vcf"]
    env0 = dict(os.environ, MALVA_GENO_BF_BITS=str(1 << 26), MALVA_GENO_BATCH="400")
    _cli(["index"] + common + [str(data / "s0")], env=env0)

    def run(opts, group, d, env, table):
        assert _cli(["call", "--cohort"] + opts + group + ["--merged", str(d / "m.vcf")] + (["--ld", str(d / "ld.tsv")] if table else []) + common +
                    [str(data / "cohort.tsv")], env=dict(env0, **env)) == ""
    tables = _check_ld_cohort(run, [(["--cohort-group", "2"], "7"), ([], "7"), (["--cohort-group", "2"], "400")], tmp_path, [], {})
    rows = _lines(tables["all"])
    assert len(rows) > 50 and {r[7] for r in rows} >= {"+", "-"} and any(r[6] not in ("1", "0.25") for r in rows)
    d = tmp_path / "o"                                                             # -o alone, in groups of 2 + 1
    d.mkdir()
    assert _cli(["call", "--cohort", "--cohort-group", "2", "-o", str(d / "out"), "--ld", str(d / "ld.tsv")] + common + [str(data / "cohort.tsv")], env=env0) == ""
    _no_leftovers(d, ["out", "ld.tsv"])
    assert open(str(d / "ld.tsv")).read() == tables["all"]
    assert not [f for f in os.listdir(data) if f.endswith(".part")]


def test_cli_ld_usage_errors_write_nothing(haploid_cohort, tmp_path):
    import subprocess
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    ld = str(tmp_path / "ld.tsv")
    base = ["call"] + COMMON + ["--cohort", "--merged", str(tmp_path / "m.vcf")]
    bad = [base + ["--ld-window", "5"],                                            # a sub-option without --ld
           base + ["--ld-window-bp", "5"], base + ["--ld-min-r2", "0.5"], base + ["--ld-min-n", "3"],
           base + ["--ld", ld, "--ld-window", "0"], base + ["--ld", ld, "--ld-window", "1025"], base + ["--ld", ld, "--ld-window", "x"],
           base + ["--ld", ld, "--ld-window", "-3"], base + ["--ld", ld, "--ld-window-bp", "-1"], base + ["--ld", ld, "--ld-window-bp", "1e6"],
           base + ["--ld", ld, "--ld-min-r2", "1.5"], base + ["--ld", ld, "--ld-min-r2", "-0.1"], base + ["--ld", ld, "--ld-min-r2", "nan"],
           base + ["--ld", ld, "--ld-min-r2", "0.5x"], base + ["--ld", ld, "--ld-min-n", "0"], base + ["--ld", ld, "--ld-min-n", "4294967296"],
           base + ["--ld", ""],
           ["call"] + COMMON + ["--ld", ld]]                                       # without --cohort
    for args in bad:
        r = subprocess.run([BIN] + args + [fa, vcf, man if "--cohort" in args else fq], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "malva : --ld" in r.stderr and r.stdout == "", args
        assert not os.listdir(tmp_path), args
