"""`call --cohort --site-stats PATH`: the per-record QC table -- genotype counts (mg_site_geno_counts) and the exact test of
Hardy-Weinberg proportions (mg_hwe_exact), both made on the device.

The ABI is compared with the restatement of tests/site_stats_model.py; the command line with that restatement applied to the merged
VCF the same run wrote -- the project's own published output, not its internals.  Every comparison is exact: the counts are integers,
and the test's doubles are compared bit for bit (every step of the definition is one correctly rounded operation in a fixed order)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from malva_amd import Context, MalvaError, synth
from site_stats_model import HEADER, geno_counts_plain, hwe_exact, site_stats_text
from test_gpu_merged import COMMON, _cli, _no_leftovers, _split, haploid_cohort  # noqa: F401 (the fixture)
from test_gpu_site_tags import _median_gq, counts_numpy
from test_sample_stats_cpu import sample_counts_plain

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE = -1, -3
MIN_GQ = 30
POISON = 0xDEADBEEF
ALLELES = (1, 2, 3, 8, 9, 70, 129)      # both sides of SITE_BALLOT_MAX (8), one and two rounds of SITE_BINS (128)
PAD = 8


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


# ---- the ABI: counts ---------------------------------------------------------------------------------------------------------------

def _cells_case(planes, n, seed):
    """records of 1, 2, 3, 8, 9, 70 and 129 alleles in turn (the turn starts where `planes` says), allele indexes -1 .. A inclusive
    (mostly inside), GQ on both sides of MIN_GQ"""
    rng = np.random.default_rng(seed)
    A = np.array([ALLELES[(v + planes) % len(ALLELES)] for v in range(n)], dtype=np.int64)
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)

    def draw():
        g = (rng.random((planes, n)) * A[None, :]).astype(np.int64)
        stray = rng.random((planes, n)) < 0.1
        g[stray] = np.where(rng.random(int(stray.sum())) < 0.5, -1, np.broadcast_to(A[None, :], (planes, n))[stray])
        zero = rng.random((planes, n)) < 0.3
        g[zero] = 0
        return g.astype(np.int32)
    g1, g2 = draw(), draw()
    same = rng.random((planes, n)) < 0.3
    g2[same] = g1[same]
    gq = rng.integers(MIN_GQ - 20, MIN_GQ + 20, size=(planes, n)).astype(np.int32)
    if n:
        gq[0, 0], gq[planes - 1, n - 1] = MIN_GQ, MIN_GQ - 1
    return g1, g2, gq, vao


@pytest.fixture(scope="module")
def cases():
    """cells and their counts by numpy, made once per (planes, n, haploid, masked) and left unchanged"""
    made = {}

    def get(planes, n, haploid, masked):
        key = (planes, n, haploid, masked)
        if key not in made:
            cells = made.get(("cells", planes, n))
            if cells is None:
                cells = made[("cells", planes, n)] = _cells_case(planes, n, seed=planes * 1000 + n)
                for x in cells:
                    x.setflags(write=False)
            g1, g2, gq, vao = cells
            want = geno_counts_plain(g1, None if haploid else g2, gq, haploid, vao, MIN_GQ if masked else None)
            for x in want:
                x.setflags(write=False)
            made[key] = cells + (want,)
        return made[key]
    return get


def _device_counts(ctx, g1, g2, gq, vao, haploid, masked, accumulate, start):
    """the device form into buffers filled with `start` (an int, or three arrays), PAD guard words on both sides -> (n, het, hom)"""
    dev = torch.device("cuda", 0)
    planes, nv = g1.shape
    slots = int(vao[nv])
    t = lambda a: torch.from_numpy(np.array(a if a.size else np.zeros(1, a.dtype)).view(np.int32)).to(dev)
    d1, d2, dq, dv = t(g1), t(g2), t(gq), t(vao)
    bufs = []
    for i, size in enumerate((nv, slots, slots)):
        h = np.full(size + 2 * PAD, POISON, dtype=np.uint32)
        if not isinstance(start, int):
            h[PAD:PAD + size] = start[i]
        bufs.append(t(h))
    torch.cuda.synchronize()
    ctx.site_geno_counts_device(nv, planes, haploid, d1.data_ptr(), 0 if haploid else d2.data_ptr(), dq.data_ptr() if masked else 0, dv.data_ptr(),
                                *(b.data_ptr() + 4 * PAD for b in bufs), min_gq=MIN_GQ if masked else None, accumulate=accumulate)
    ctx.synchronize()
    out = []
    for b, size in zip(bufs, (nv, slots, slots)):
        h = b.cpu().numpy().view(np.uint32)
        assert (h[:PAD] == POISON).all() and (h[PAD + size:] == POISON).all(), "written outside the records' slots"
        out.append(h[PAD:PAD + size].copy())
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("haploid", [False, True])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257])
@pytest.mark.parametrize("planes", [1, 2, 63, 64])
def test_counts_equal_the_model(ctx, cases, planes, n, haploid, masked):
    g1, g2, gq, vao, want = cases(planes, n, haploid, masked)
    q = MIN_GQ if masked else None
    got = ctx.site_geno_counts(g1, None if haploid else g2, gq if masked else None, haploid, vao, min_gq=q)
    for g, w, what in zip(got, want, ("n", "het", "hom")):
        assert np.array_equal(g, w), what
    if haploid:
        assert not got[1].any()
    # the device form, every output poisoned: every slot of every record is written, nothing beyond
    dev = _device_counts(ctx, g1, g2, gq, vao, haploid, masked, False, POISON)
    for g, w, what in zip(dev, want, ("n", "het", "hom")):
        assert np.array_equal(g, w), "device form: " + what
    # accumulate: on top of what the arrays hold, in both forms
    rng = np.random.default_rng(n + planes)
    start = [rng.integers(0, 1000, size=w.size).astype(np.uint32) for w in want]
    acc = [s.copy() for s in start]
    ctx.site_geno_counts(g1, None if haploid else g2, gq if masked else None, haploid, vao, min_gq=q, n=acc[0], het=acc[1], hom=acc[2])
    dev = _device_counts(ctx, g1, g2, gq, vao, haploid, masked, True, start)
    for a, d, s, w in zip(acc, dev, start, want):
        assert np.array_equal(a, s + w) and np.array_equal(d, s + w)


def test_counts_differ_from_the_site_tags_where_one_index_is_invalid(ctx):
    """0/2 in a record of two alleles: mg_site_counts counts the 0, mg_site_geno_counts nothing"""
    g1, g2, gq, vao = (np.array([[0], [1]], dtype=np.int32), np.array([[2], [1]], dtype=np.int32), np.zeros((2, 1), dtype=np.int32), np.array([0, 2], dtype=np.uint32))
    ac, ns = ctx.site_counts(g1, g2, gq, False, vao)
    n, het, hom = ctx.site_geno_counts(g1, g2, None, False, vao)
    assert ac.tolist() == [1, 2] and ns.tolist() == [2]
    assert (n.tolist(), het.tolist(), hom.tolist()) == ([1], [0, 0], [0, 1])


# ---- the ABI: the test -------------------------------------------------------------------------------------------------------------

def _items():
    """1000 items: the directed values, the seams of the walk, NaN items among valid ones, one item of 16,384 individuals, random ones"""
    items = [(0, 0, 0), (1, 1, 0), (3, 3, 0), (100, 21, 4), (2, 1, 2), (16384, 16384, 0), (0, 1, 0), (5, 0, 6),
             (7, 0, 0), (7, 0, 7),            # r = 0: mid at 0 and at r, the single term
             (9, 1, 0), (9, 1, 8),            # r = 1: mid raised to r
             (10, 2, 0), (10, 0, 1),          # r = 2 (even): het = r, het = 0
             (10, 3, 0), (10, 1, 1),          # r = 3 (odd): het = r, het = 1
             (40, 0, 20), (40, 40, 0), (40, 20, 10), (41, 21, 10), (1000, 0, 20), (1000, 40, 0),
             (16384, 8192, 4096), (1 << 24, 0, 0), ((1 << 24) + 1, 0, 0), (4, 5, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)]
    rng = np.random.default_rng(11)
    while len(items) < 1000:
        n = int(rng.integers(0, 300))
        het = int(rng.integers(0, n + 1))
        hom = int(rng.integers(0, n - het + 1))
        if rng.random() < 0.03:
            hom = n - het + 1 + int(rng.integers(0, 3))                            # het + hom > n
        items.append((n, het, hom))
    return items


@pytest.fixture(scope="module")
def hwe_cases():
    items = np.array(_items(), dtype=np.uint32)
    want = np.array([hwe_exact(*(int(x) for x in it)) for it in items], dtype=np.float64)
    items.setflags(write=False)
    want.setflags(write=False)
    nan = np.isnan(want[:, 0])
    assert nan.sum() >= 10 and (np.isnan(want[:, 1]) == nan).all() and not nan[:4].any() and nan[4]
    assert want[5].tolist() == [0.0, 0.0] and want[0].tolist() == [1.0, 1.0]
    return items, want


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n_items", [0, 1, 63, 64, 65, 1000])
def test_hwe_is_the_model_bit_for_bit(ctx, hwe_cases, n_items):
    items, want = hwe_cases
    it, w = items[:n_items], want[:n_items]
    hwe, exc = ctx.hwe_exact(it[:, 0], it[:, 1], it[:, 2])
    bad = np.flatnonzero((_bits(hwe) != _bits(w[:, 0])) | (_bits(exc) != _bits(w[:, 1])))
    assert bad.size == 0, [(it[i].tolist(), hwe[i], w[i, 0], exc[i], w[i, 1]) for i in bad[:5]]
    # the device form into poisoned buffers
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.array(a if a.size else np.zeros(1, a.dtype)).view(np.int32)).to(dev)
    dn, dh, do = (t(it[:, k]) for k in range(3))
    outs = [torch.full((n_items + 2 * PAD,), -7.5, dtype=torch.float64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    ctx.hwe_exact_device(n_items, dn.data_ptr(), dh.data_ptr(), do.data_ptr(), *(o.data_ptr() + 8 * PAD for o in outs))
    ctx.synchronize()
    for o, k in zip(outs, (0, 1)):
        h = o.cpu().numpy()
        assert (h[:PAD] == -7.5).all() and (h[PAD + n_items:] == -7.5).all()
        assert np.array_equal(_bits(h[PAD:PAD + n_items]), _bits(w[:, k]))


# ---- arguments, the timer, the neighbours -------------------------------------------------------------------------------------------

def test_argument_errors(ctx):
    g = np.zeros((3, 2), dtype=np.int32)
    vao = np.array([0, 2, 4], dtype=np.uint32)
    n, het, hom = np.zeros(2, dtype=np.uint32), np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L, h = ctx._L, ctx.h
    call = lambda planes, hap, g1, g2, gq, mask, vo, no, he, ho: L.mg_site_geno_counts(h, 2, planes, hap, g1, g2, gq, mask, 0, vo, 0, no, he, ho)
    assert call(3, 0, p(g), p(g), None, 0, p(vao), p(n), p(het), p(hom)) == 0
    assert call(3, 1, p(g), None, None, 0, p(vao), p(n), p(het), p(hom)) == 0      # haploid: no gt2
    for planes in (0, 65):
        assert call(planes, 0, p(g), p(g), None, 0, p(vao), p(n), p(het), p(hom)) == MG_ERR_ARG
    assert call(3, 0, None, p(g), None, 0, p(vao), p(n), p(het), p(hom)) == MG_ERR_ARG
    assert call(3, 0, p(g), None, None, 0, p(vao), p(n), p(het), p(hom)) == MG_ERR_ARG
    assert call(3, 0, p(g), p(g), None, 1, p(vao), p(n), p(het), p(hom)) == MG_ERR_ARG  # the mask needs gq
    assert call(3, 0, p(g), p(g), None, 0, None, p(n), p(het), p(hom)) == MG_ERR_ARG
    assert call(3, 0, p(g), p(g), None, 0, p(vao), None, p(het), p(hom)) == MG_ERR_ARG
    assert call(3, 0, p(g), p(g), None, 0, p(vao), p(n), None, p(hom)) == MG_ERR_ARG
    assert call(3, 0, p(g), p(g), None, 0, p(vao), p(n), p(het), None) == MG_ERR_ARG
    assert L.mg_site_geno_counts(h, 0, 3, 0, None, None, None, 0, 0, None, 0, None, None, None) == 0   # no records: nothing is read
    assert L.mg_site_geno_counts_device(h, 2, 0, 1, None, None, None, 0, 0, None, 0, None, None, None) == MG_ERR_ARG
    with pytest.raises(MalvaError, match="n_planes"):
        ctx.site_geno_counts(np.zeros((65, 2), dtype=np.int32), None, None, True, vao)
    x, out = np.ones(2, dtype=np.uint32), np.zeros(2, dtype=np.float64)
    assert L.mg_hwe_exact(h, 2, p(x), p(x), p(x), p(out), p(out.copy())) == 0
    for k in range(5):
        args = [p(x), p(x), p(x), p(out), p(out)]
        args[k] = None
        assert L.mg_hwe_exact(h, 2, *args) == MG_ERR_ARG
        assert L.mg_hwe_exact_device(h, 2, *args) == MG_ERR_ARG
    assert L.mg_hwe_exact(h, 0, None, None, None, None, None) == 0
    assert L.mg_hwe_stats(h, None) == MG_ERR_ARG


def test_hwe_stats_before_the_first_call():
    with Context(35, 43, 1 << 20) as c:
        ms = (C.c_float * 2)(5.0, 5.0)
        assert c._L.mg_hwe_stats(c.h, ms) == MG_ERR_STATE
        with pytest.raises(MalvaError) as e:
            c.hwe_stats()
        assert e.value.code == MG_ERR_STATE
        c.hwe_exact(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32))
        ms = c.hwe_stats()                                                         # no items: the call still counts as one
        assert ms[0] == 0 and ms[1] >= 0
        c.site_geno_counts(np.zeros((2, 0), dtype=np.int32), None, None, True, np.zeros(1, dtype=np.uint32))
        assert all(m >= 0 for m in c.hwe_stats())


def test_the_site_table_calls_and_their_neighbours_do_not_disturb_each_other(cases, hwe_cases):
    """one context: the neighbours, the two calls, the neighbours again -- every result what it is alone; a call of one kind leaves the
    timers of the others what they were"""
    planes, n = 3, 257
    g1, g2, gq, vao, want = cases(planes, n, False, True)
    items, want_p = hwe_cases
    items, want_p = items[:65], want_p[:65]
    want_ac, want_ns = counts_numpy(g1, g2, gq, False, vao, MIN_GQ)
    want_table = sample_counts_plain(g1, g2, gq, False, vao, None, None, None, MIN_GQ)
    with Context(35, 43, 1 << 20) as c:
        def neighbours():
            ac, ns = c.site_counts(g1, g2, gq, False, vao, min_gq=MIN_GQ)
            table = c.sample_counts(g1, g2, gq, False, vao, min_gq=MIN_GQ)
            assert np.array_equal(ac, want_ac) and np.array_equal(ns, want_ns) and np.array_equal(table, want_table)
            return c.site_stats() + (c.sample_stats(),)
        before = neighbours()
        got = c.site_geno_counts(g1, g2, gq, False, vao, min_gq=MIN_GQ)
        ms_counts = c.hwe_stats()
        hwe, exc = c.hwe_exact(items[:, 0], items[:, 1], items[:, 2])
        assert c.site_stats() + (c.sample_stats(),) == before, "the site table's calls changed a neighbour's timer"
        ms = c.hwe_stats()
        assert ms[0] == ms_counts[0], "mg_hwe_exact changed the timer of mg_site_geno_counts"
        assert all(m >= 0 for m in neighbours()) and c.hwe_stats() == ms, "a neighbour changed mg_hwe_stats"
        again = c.site_geno_counts(g1, g2, gq, False, vao, min_gq=MIN_GQ)
        for a, b, w in zip(got, again, want):
            assert np.array_equal(a, w) and np.array_equal(b, w)
        assert np.array_equal(_bits(hwe), _bits(want_p[:, 0])) and np.array_equal(_bits(exc), _bits(want_p[:, 1]))
        neighbours()


# ---- the command line -------------------------------------------------------------------------------------------------------------

def table_from_vcf(text, min_gq):
    """the table the model makes from a merged VCF: GT and GQ of the cells; a masked cell shows no indexes and is not usable"""
    head, recs = _split(text)
    S, n = len(head[-1].split("\t")[9:]), len(recs)
    g1, g2 = (np.full((S, n), -1, dtype=np.int64) for _ in range(2))
    gq = np.zeros((S, n), dtype=np.int64)
    vao, cols5, diploid = [0], [], False
    for v, rec in enumerate(recs):
        cols = rec.split("\t")
        assert cols[8].startswith("GT:GQ")
        vao.append(vao[-1] + 1 + (0 if cols[4] == "." else len(cols[4].split(","))))
        cols5.append("\t".join(cols[:5]))
        for s, cell in enumerate(cols[9:]):
            gt, q = cell.split(":")[:2]
            gq[s, v] = int(q)
            diploid = diploid or "/" in gt
            if "." in gt:
                assert min_gq is not None and int(q) < min_gq
            else:
                assert min_gq is None or int(q) >= min_gq
                al = [int(a) for a in gt.split("/")]
                g1[s, v], g2[s, v] = al[0], al[-1]
    n_usable, het, hom = geno_counts_plain(g1, g2, gq, not diploid, vao, min_gq)
    return site_stats_text(cols5, S, not diploid, vao, n_usable, het, hom)


def _rows(table):
    lines = table.split("\n")
    assert lines[-1] == "" and lines[0] + "\n" == HEADER
    return [l.split("\t") for l in lines[1:-1]]


def _check_cohort(run, groups, tmp_path):
    """run(opts, group, directory, env, table) writes directory/m.vcf and, if table, directory/t.tsv; groups: the grouped runs that must
    give the same bytes"""
    tables = {}
    q = None
    for tag in ("all", "masked"):
        opts = [] if q is None else ["--min-gq", str(q)]
        d = tmp_path / tag
        d.mkdir()
        run(opts, [], d, {}, True)
        _no_leftovers(d, ["m.vcf", "t.tsv"])
        merged = open(str(d / "m.vcf")).read()
        table = open(str(d / "t.tsv")).read()
        assert table == table_from_vcf(merged, q), tag
        assert len(_rows(table)) == sum(r.split("\t")[4] != "." for r in _split(merged)[1]) > 0
        tables[tag] = table
        for i, group in enumerate(groups):                                         # whatever the grouping and the batches: the same bytes
            g = tmp_path / ("%s-g%d" % (tag, i))
            g.mkdir()
            run(opts, group, g, {"MALVA_GENO_BATCH": "7"}, True)
            _no_leftovers(g, ["m.vcf", "t.tsv"])
            assert open(str(g / "t.tsv")).read() == table, "%s %s" % (tag, group)
            assert open(str(g / "m.vcf")).read() == merged
        if q is None:
            plain = tmp_path / "plain"                                             # without --site-stats: the same merged file
            plain.mkdir()
            run(opts, [], plain, {}, False)
            _no_leftovers(plain, ["m.vcf"])
            assert open(str(plain / "m.vcf")).read() == merged
            q = _median_gq(merged)
    assert tables["all"] != tables["masked"], "--min-gq %d changes nothing in the table" % q
    return tables


def test_cli_site_stats_on_the_haploid_cohort(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    _cli(["index"] + COMMON + [fa, vcf, fq])

    def run(opts, group, d, env, table):
        assert _cli(["call"] + COMMON + opts + group + ["--cohort", "--merged", str(d / "m.vcf")] + (["--site-stats", str(d / "t.tsv")] if table else []) + [fa, vcf, man],
                    env=dict(os.environ, **env)) == ""
    tables = _check_cohort(run, [["--cohort-group", "3"], ["--cohort-group", "2"]], tmp_path)
    rows = _rows(tables["all"])
    for r in rows:                                                                 # haploid: no HET, no test; HOM is AC
        assert r[5] == "4" and r[7] == r[6] and r[10] == r[8]
        assert set(r[11].split(",")) == {"0"} and set(r[12].split(",")) == {"."} and r[13] == r[12]
    assert any(x != "0" for r in rows for x in r[8].split(",")), "no ALT allele is called"
    # -o alone, without --merged: the same table (one group, and groups of 3 + 1)
    for i, group in enumerate(([], ["--cohort-group", "3"])):
        d = tmp_path / ("o%d" % i)
        d.mkdir()
        assert _cli(["call"] + COMMON + group + ["--cohort", "-o", str(d / "out"), "--site-stats", str(d / "t.tsv"), fa, vcf, man]) == ""
        _no_leftovers(d, ["out", "t.tsv"])
        assert open(str(d / "t.tsv")).read() == tables["all"]
    _no_leftovers(tmp, ["haploid.fq", "dump.txt", "sim1.fq", "sim2.fq", "keep.txt", "cohort.tsv"] + [f for f in os.listdir(tmp) if f.startswith("haploid.vcf.gz")])


def test_cli_site_stats_on_general_blocks(tmp_path):
    """the diploid panel of tests/test_gpu_sample_stats.py::test_cli_sample_stats_on_general_blocks: multi-allelic records and
    heterozygous cells; grouped runs in batches of 7 records"""
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
        assert _cli(["call", "--cohort"] + opts + group + ["--merged", str(d / "m.vcf")] + (["--site-stats", str(d / "t.tsv")] if table else []) + common +
                    [str(data / "cohort.tsv")], env=dict(env0, **env)) == ""
    tables = _check_cohort(run, [["--cohort-group", "3"], ["--cohort-group", "2"]], tmp_path)
    rows = _rows(tables["all"])
    assert any(x != "0" for r in rows for x in r[11].split(",")), "no heterozygote"
    assert any("," in r[4] and r[12].count(",") == r[4].count(",") for r in rows), "no multi-allelic line"
    assert any(x not in ("1", ".") for r in rows for x in r[12].split(",")), "every HWE is 1 or ."
    d = tmp_path / "o"                                                             # -o alone, in groups of 2 + 1
    d.mkdir()
    assert _cli(["call", "--cohort", "--cohort-group", "2", "-o", str(d / "out"), "--site-stats", str(d / "t.tsv")] + common + [str(data / "cohort.tsv")], env=env0) == ""
    _no_leftovers(d, ["out", "t.tsv"])
    assert open(str(d / "t.tsv")).read() == tables["all"]
    assert not [f for f in os.listdir(data) if f.endswith(".part")]
