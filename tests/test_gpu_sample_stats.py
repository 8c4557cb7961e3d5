"""`call --cohort --sample-stats PATH`: the per-sample QC table, summed on the device (mg_sample_counts).

The ABI is compared with the numpy restatement of tests/test_sample_stats_cpu.py; the command line with that restatement applied
to the merged VCF the same run wrote -- the project's own published output, not its internals.  Every comparison is exact: the
results are integers, and the five ratios of the text are one double division each."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from malva_amd import Context, MalvaError, synth
from malva_amd.capi import SAMPLE_SLOTS
from test_gpu_merged import COMMON, _cli, _no_leftovers, _split, format_plain, haploid_cohort  # noqa: F401 (the fixture)
from test_gpu_site_tags import _median_gq, counts_numpy
from test_pairs_cpu import pack_plain
from test_sample_stats_cpu import COLUMNS, SLOT_NAMES, SS, allele_class_plain, sample_counts_plain, sample_stats_text

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE = -1, -3
MIN_GQ = 30
POISON = np.uint64(0xDEADBEEFDEADBEEF)
STATUS_SLOTS = [SS[k] for k in ("NORMAL", "OVERCOV", "SINGLE", "NOCOV")]
CLASS_SLOTS = [SS[k] for k in ("TS", "TV", "INS", "DEL", "OTHER")]


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------

def _cells_case(planes, n, seed):
    """records of 1, 2, 3, 9 and 70 alleles (mostly 2), allele indexes -1 .. A inclusive (mostly inside), GQ in [-5, 300], coverages
    up to 2^32 - 1, status in {0, 1, 2, 3, 7}, classes 0 .. 7 on every slot (slot 0 of a record is never looked up)"""
    rng = np.random.default_rng(seed)
    A = rng.choice(np.array([1, 2, 3, 9, 70]), size=n, p=[0.08, 0.8, 0.08, 0.03, 0.01])
    if n >= 5:
        A[:5] = (1, 2, 3, 9, 70)
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)

    def draw():
        g = (rng.random((planes, n)) * A[None, :]).astype(np.int64)              # 0 .. A - 1
        stray = rng.random((planes, n)) < 0.1
        g[stray] = np.where(rng.random(int(stray.sum())) < 0.5, -1, np.broadcast_to(A[None, :], (planes, n))[stray])
        zero = rng.random((planes, n)) < 0.4
        g[zero] = 0
        return g.astype(np.int32)
    g1, g2 = draw(), draw()
    gq = rng.integers(-5, 301, size=(planes, n)).astype(np.int32)
    if n >= 3:
        gq[0, :3], gq[planes - 1, -3:] = (-5, 300, MIN_GQ), (MIN_GQ - 1, 99, 100)
    cov = rng.integers(0, 1 << 32, size=(planes, int(vao[-1])), dtype=np.uint64)
    cov[rng.random(cov.shape) < 0.2] = (1 << 32) - 1
    cov[rng.random(cov.shape) < 0.2] = 0
    status = rng.choice(np.array([0, 1, 2, 3, 7], dtype=np.uint8), size=(planes, n))
    cls = rng.integers(0, 8, size=int(vao[-1])).astype(np.uint8)
    return g1, g2, gq, vao, status, cov.astype(np.uint32), cls


@pytest.fixture(scope="module")
def cases():
    """cells and their table by numpy, made once per (planes, n, haploid, masked) and left unchanged"""
    made = {}

    def get(planes, n, haploid, masked):
        key = (planes, n, haploid, masked)
        if key not in made:
            cells = made.get(("cells", planes, n))
            if cells is None:
                cells = made[("cells", planes, n)] = _cells_case(planes, n, seed=planes * 1000 + n % 997)
                for x in cells:
                    x.setflags(write=False)
            g1, g2, gq, vao, status, cov, cls = cells
            want = sample_counts_plain(g1, g2, gq, haploid, vao, status, cov, cls, MIN_GQ if masked else None)
            want.setflags(write=False)
            made[key] = cells + (want,)
        return made[key]
    return get


def _has_what_it_is_meant_to_have(g1, g2, gq, vao, status, cov, cls, want, haploid, masked):
    A = np.diff(vao.astype(np.int64))
    assert all((A == a).any() for a in (1, 2, 3, 9, 70))
    for g in (g1, g2):
        assert (g == -1).any() and (g == A[None, :]).any() and (g == A[None, :] - 1).any() and (g == 0).any()
    assert gq.min() == -5 and gq.max() == 300 and (gq < MIN_GQ).any()
    assert cov.max() == (1 << 32) - 1 and (want[:, SS["COV_SUM"]] > np.uint64(1 << 32)).all()
    assert all((status == s).any() for s in (0, 1, 2, 3, 7))
    assert all(want[:, k].any() for k in range(len(SLOT_NAMES)) if not (haploid and SLOT_NAMES[k] in ("HET", "HET_ALT")) and not (not masked and SLOT_NAMES[k] == "MASKED"))


def _run(ctx, case, haploid, masked, **kw):
    g1, g2, gq, vao, status, cov, cls = case[:7]
    return ctx.sample_counts(g1, None if haploid else g2, gq, haploid, vao, status, cov, cls, min_gq=MIN_GQ if masked else None, **kw)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize("masked", [False, True], ids=["all-called", "masked"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 3, 64])
def test_counts_are_exact(ctx, cases, planes, haploid, masked, n):
    case = cases(planes, n, haploid, masked)
    want = case[-1]
    if n >= 257:
        _has_what_it_is_meant_to_have(*case, haploid, masked)
    got = _run(ctx, case, haploid, masked)
    assert got.shape == (planes, SAMPLE_SLOTS) and np.array_equal(got, want), [SLOT_NAMES[k] for k in np.nonzero((got != want).any(axis=0))[0] if k < len(SLOT_NAMES)]
    assert np.array_equal(got[:, SS["RECORDS"]], got[:, SS["MASKED"]] + got[:, SS["BAD"]] + got[:, SS["CALLED"]]) and (got[:, SS["RECORDS"]] == n).all()
    ms = ctx.sample_stats()
    assert np.isfinite(ms) and ms >= 0


def test_a_wave_that_takes_several_steps(ctx, cases):
    """64 planes leave 32 runs to a plane: 20,011 records are 79 chunks of 256, three to a workgroup and a last run of 43 records"""
    case = cases(64, 20011, False, True)
    assert np.array_equal(_run(ctx, case, False, True), case[-1])


@pytest.mark.parametrize("planes,n", [(3, 65), (64, 5000)])
def test_accumulate(ctx, cases, planes, n):
    case = cases(planes, n, False, True)
    g1, g2, gq, vao, status, cov, cls, want = case
    # two halves summed are the whole
    cut = (n * 5) // 13
    a0 = int(vao[cut])
    vlo, vhi = vao[:cut + 1], vao[cut:] - vao[cut]
    two = ctx.sample_counts(g1[:, :cut], g2[:, :cut], gq[:, :cut], False, vlo, status[:, :cut], cov[:, :a0], cls[:a0], min_gq=MIN_GQ)
    assert ctx.sample_counts(g1[:, cut:], g2[:, cut:], gq[:, cut:], False, vhi, status[:, cut:], cov[:, a0:], cls[a0:], min_gq=MIN_GQ, counts=two) is two
    assert np.array_equal(two, want)
    # accumulate == 0 over a poisoned table overwrites all 32 slots of every plane, the reserved ones with 0
    poisoned = np.full((planes, SAMPLE_SLOTS), POISON, dtype=np.uint64)
    assert _run(ctx, case, False, True, counts=poisoned, overwrite=True) is poisoned and np.array_equal(poisoned, want)
    assert not poisoned[:, len(SLOT_NAMES):].any()
    # ... and with accumulate they are left alone
    kept = want.copy()
    kept[:, len(SLOT_NAMES):] = POISON
    _run(ctx, case, False, True, counts=kept)
    assert np.array_equal(kept[:, :len(SLOT_NAMES)], 2 * want[:, :len(SLOT_NAMES)]) and (kept[:, len(SLOT_NAMES):] == POISON).all()
    # the planes at and beyond n_planes of a larger buffer keep what they hold, with and without accumulate; no records: zeros
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    for acc in (0, 1):
        for n_vars in (n, 0):
            big = np.full((planes + 2, SAMPLE_SLOTS), POISON, dtype=np.uint64)
            if acc:
                big[:planes] = 0
            ctx._ck(ctx._L.mg_sample_counts(ctx.h, n_vars, planes, 0, p(g1), p(g2), p(gq), 1, MIN_GQ, p(status), p(cov), p(vao), p(cls), acc, p(big)))
            assert np.array_equal(big[:planes], want if n_vars else np.zeros_like(want)) and (big[planes:] == POISON).all()


@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
def test_the_optional_arrays_one_at_a_time(ctx, cases, haploid):
    g1, g2, gq, vao, status, cov, cls, want = cases(3, 257, haploid, True)
    g2 = None if haploid else g2
    for missing, slots in (("status", STATUS_SLOTS), ("cov", [SS["COV_SUM"]]), ("allele_class", CLASS_SLOTS)):
        kw = dict(status=status, cov=cov, allele_class=cls)
        kw[missing] = None
        got = ctx.sample_counts(g1, g2, gq, haploid, vao, min_gq=MIN_GQ, **kw)
        expect = want.copy()
        assert expect[:, slots].any()
        expect[:, slots] = 0
        assert np.array_equal(got, expect), missing
        assert np.array_equal(got, sample_counts_plain(g1, g2, gq, haploid, vao, min_gq=MIN_GQ, **kw))
        # with accumulate the slots of a missing array keep what they hold
        start = np.full((3, SAMPLE_SLOTS), 5, dtype=np.uint64)
        ctx.sample_counts(g1, g2, gq, haploid, vao, min_gq=MIN_GQ, counts=start, **kw)
        assert np.array_equal(start[:, :len(SLOT_NAMES)], expect[:, :len(SLOT_NAMES)] + np.uint64(5)) and (start[:, len(SLOT_NAMES):] == 5).all()


@pytest.mark.parametrize("planes,n", [(3, 257), (64, 5000), (1, 65)])
def test_device_form_equals_the_host_form(cases, planes, n):
    """on torch tensors, the context on a stream that is not the default one"""
    g1, g2, gq, vao, status, cov, cls, want = cases(planes, n, False, True)
    dev = torch.device("cuda", 0)
    v = C.c_void_p
    with Context(35, 43, 1 << 20) as c:
        side = torch.cuda.Stream(device=dev)
        c.set_stream(side.cuda_stream)
        d1, d2, dq, dv, dc = (torch.from_numpy(np.array(x).view(np.int32)).to(dev) for x in (g1, g2, gq, vao, cov))
        ds, dk = (torch.from_numpy(np.array(x)).to(dev) for x in (status, cls))
        guard = 64
        counts = torch.full((guard + planes * SAMPLE_SLOTS + guard,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        d_counts = counts.data_ptr() + 8 * guard
        args = (c.h, n, planes, 0, v(d1.data_ptr()), v(d2.data_ptr()), v(dq.data_ptr()), 1, MIN_GQ, v(ds.data_ptr()), v(dc.data_ptr()), v(dv.data_ptr()), v(dk.data_ptr()))
        c._ck(c._L.mg_sample_counts_device(*args, 0, v(d_counts)))
        c.synchronize()
        once = counts.cpu().numpy()
        c._ck(c._L.mg_sample_counts_device(*args, 1, v(d_counts)))
        c.synchronize()
        twice = counts.cpu().numpy()
        for h in (once, twice):
            assert (h[:guard] == 0x5A5A5A5A).all() and (h[-guard:] == 0x5A5A5A5A).all(), "words outside the table were written"
        host = c.sample_counts(g1, g2, gq, False, vao, status, cov, cls, min_gq=MIN_GQ)
        assert np.array_equal(host, want)
        assert np.array_equal(once[guard:-guard].view(np.uint64).reshape(planes, SAMPLE_SLOTS), host)
        assert np.array_equal(twice[guard:-guard].view(np.uint64).reshape(planes, SAMPLE_SLOTS), 2 * host)
        assert c.sample_stats() >= 0


def test_arguments(ctx):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    g = np.zeros((65, 2), dtype=np.int32)
    st = np.zeros((65, 2), dtype=np.uint8)
    vao = np.array([0, 2, 4], dtype=np.uint32)
    cov = np.zeros((65, 4), dtype=np.uint32)
    cls = np.zeros(4, dtype=np.uint8)
    out = np.zeros((65, SAMPLE_SLOTS), dtype=np.uint64)
    call = lambda n, planes, hap, g1, g2, gq, vo, counts: ctx._L.mg_sample_counts(ctx.h, n, planes, hap, g1, g2, gq, 0, 0, p(st), p(cov), vo, p(cls), 0, counts)
    for planes in (0, 65):
        assert call(2, planes, 0, p(g), p(g), p(g), p(vao), p(out)) == MG_ERR_ARG
    assert call(2, 3, 0, p(g), p(g), p(g), p(vao), None) == MG_ERR_ARG                 # counts
    assert call(2, 3, 0, None, p(g), p(g), p(vao), p(out)) == MG_ERR_ARG               # gt1
    assert call(2, 3, 0, p(g), p(g), None, p(vao), p(out)) == MG_ERR_ARG               # gq: read with or without the mask
    assert call(2, 3, 0, p(g), p(g), p(g), None, p(out)) == MG_ERR_ARG                 # var_allele_off
    assert call(2, 3, 0, p(g), None, p(g), p(vao), p(out)) == MG_ERR_ARG               # diploid: gt2 is read
    assert call(2, 3, 1, p(g), None, p(g), p(vao), p(out)) == 0                        # haploid: it is not
    out[:] = 7
    assert call(0, 3, 0, None, None, None, None, p(out)) == 0                          # no records: the entries are zeroed
    assert not out[:3].any() and (out[3:] == 7).all()
    assert ctx._L.mg_sample_counts(ctx.h, 2, 3, 1, p(g), None, p(g), 0, 0, None, None, p(vao), None, 0, p(out)) == 0   # the optional arrays
    assert ctx._L.mg_sample_counts_device(ctx.h, 2, 0, 1, None, None, None, 0, 0, None, None, None, None, 0, None) == MG_ERR_ARG
    with pytest.raises(MalvaError, match="n_planes"):
        ctx.sample_counts(g, g, g, False, vao)


def test_sample_stats_before_the_first_call():
    with Context(35, 43, 1 << 20) as c:
        ms = (C.c_float * 1)(5.0)
        assert c._L.mg_sample_stats(c.h, ms) == MG_ERR_STATE
        with pytest.raises(MalvaError) as e:
            c.sample_stats()
        assert e.value.code == MG_ERR_STATE
        c.sample_counts(np.zeros((2, 0), dtype=np.int32), None, np.zeros((2, 0), dtype=np.int32), True, np.zeros(1, dtype=np.uint32))
        assert c.sample_stats() >= 0                                               # no records: the call still counts as one


def test_the_sample_call_and_its_neighbours_do_not_disturb_each_other(cases):
    """one context: every neighbour, the sample table, every neighbour again -- every result what it is alone; a call of one kind leaves
    the timers of the others what they were"""
    planes, n = 3, 257
    g1, g2, gq, vao, status, cov, cls, want = cases(planes, n, False, True)
    g1, g2 = np.clip(g1, 0, 1), np.clip(g2, 0, 1)                                  # (the text formatter of the test takes what a call gives)
    want = sample_counts_plain(g1, g2, gq, False, vao, status, cov, cls, MIN_GQ)
    want_planes = pack_plain(g1, g2, gq, False, vao, MIN_GQ)
    want_ac, want_ns = counts_numpy(g1, g2, gq, False, vao, MIN_GQ)
    want_text = format_plain(g1, g2, gq, False)
    with Context(35, 43, 1 << 20) as c:
        def neighbours():
            packed = c.pack_dosage(g1, g2, gq, False, vao, min_gq=MIN_GQ)
            ac, ns = c.site_counts(g1, g2, gq, False, vao, min_gq=MIN_GQ)
            text, off = c.format_calls(g1, g2, gq, False)
            assert np.array_equal(packed, want_planes) and np.array_equal(ac, want_ac) and np.array_equal(ns, want_ns)
            assert text == want_text[0] and np.array_equal(off, want_text[1])
            return c.pairs_stats() + c.site_stats() + c.format_stats()
        before = neighbours()
        got = c.sample_counts(g1, g2, gq, False, vao, status, cov, cls, min_gq=MIN_GQ)
        assert c.pairs_stats() + c.site_stats() + c.format_stats() == before, "mg_sample_counts changed a neighbour's timer"
        ms = c.sample_stats()
        assert all(m >= 0 for m in neighbours()) and c.sample_stats() == ms, "a neighbour changed mg_sample_stats"
        c.sample_counts(g1, g2, gq, False, vao, status, cov, cls, min_gq=MIN_GQ, counts=got)
        assert np.array_equal(got, 2 * want)
        neighbours()


# ---- the command line -------------------------------------------------------------------------------------------------------------

def counts_from_vcf(text, min_gq):
    """-> (names, counts [S, 32] without the status slots) from a merged VCF written with -v: GT, GQ and COVS of the cells, the allele
    classes from REF / ALT"""
    head, recs = _split(text)
    names = head[-1].split("\t")[9:]
    S, n = len(names), len(recs)
    g1, g2, gq = (np.zeros((S, n), dtype=np.int64) for _ in range(3))
    vao, cls, cov, diploid = [0], [], [[] for _ in names], False
    for v, rec in enumerate(recs):
        cols = rec.split("\t")
        assert cols[8] == "GT:GQ:COVS"
        alts = [] if cols[4] == "." else cols[4].split(",")
        vao.append(vao[-1] + 1 + len(alts))
        cls += [0] + [allele_class_plain(cols[3], a) for a in alts]
        for s, cell in enumerate(cols[9:]):
            gt, q, covs = cell.split(":")
            gq[s, v] = int(q)
            cv = [int(x) & 0xFFFFFFFF for x in covs.split(",")]
            assert len(cv) == 1 + len(alts)
            cov[s] += cv
            diploid = diploid or "/" in gt
            if "." in gt:                                                          # masked: the indexes are not shown and not needed
                assert min_gq is not None and int(q) < min_gq
            else:
                assert min_gq is None or int(q) >= min_gq
                al = [int(a) for a in gt.split("/")]
                g1[s, v], g2[s, v] = al[0], al[-1]
    return names, sample_counts_plain(g1, g2, gq, not diploid, vao, None, np.array(cov, dtype=np.uint64).reshape(S, vao[-1]), cls, min_gq)


def _table_rows(text):
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == ["#SAMPLE"] + COLUMNS + ["CALL_RATE", "HET_HOM", "TSTV", "MEAN_GQ", "MEAN_COV"]
    return [l.split("\t") for l in lines[1:-1]]


def _check_cohort(run, groups, tmp_path, diploid):
    """run(opts, group, directory, env) writes directory/m.vcf and directory/s.tsv; groups: the grouped runs that must give the same table"""
    tables = {}
    q = None
    for tag in ("all", "masked"):
        opts = [] if q is None else ["--min-gq", str(q)]
        d = tmp_path / tag
        d.mkdir()
        run(opts, [], d, {})
        _no_leftovers(d, ["m.vcf", "s.tsv"])
        merged = open(str(d / "m.vcf")).read()
        names, want = counts_from_vcf(merged, q)
        table = open(str(d / "s.tsv")).read()
        rows = _table_rows(table)
        assert [r[0] for r in rows] == names
        first = 1 + COLUMNS.index("NORMAL")
        for i, r in enumerate(rows):                                               # status: not in the merged file; the four columns cover the records
            st = [int(x) for x in r[first:first + 4]]
            assert sum(st) == int(r[1]) == len(_split(merged)[1])
            want[i, STATUS_SLOTS] = st
        assert table == sample_stats_text(names, want), tag
        col = lambda name: [int(r[1 + COLUMNS.index(name)]) for r in rows]
        assert any(col("CALLED")) and any(col("HOM_ALT")) and any(col("COV_SUM")) and any(x != "." for r in rows for x in r[-5:])
        assert any(col("MASKED")) == (q is not None)
        if diploid:
            assert any(col("HET")) and any(col("INS")) and any(col("DEL")), "the cohort shows no heterozygote or no indel"
        else:
            assert not any(col("HET")) and not any(col("HET_ALT")) and any(col("TS") + col("TV"))
        tables[tag] = table
        for i, group in enumerate(groups):                                         # whatever the grouping and the batches: the same bytes
            g = tmp_path / ("%s-g%d" % (tag, i))
            g.mkdir()
            run(opts, group, g, {"MALVA_GENO_BATCH": "7"})
            _no_leftovers(g, ["m.vcf", "s.tsv"])
            assert open(str(g / "s.tsv")).read() == table, "%s %s" % (tag, group)
            assert open(str(g / "m.vcf")).read() == merged
        if q is None:
            q = _median_gq(merged)
    assert tables["all"] != tables["masked"], "--min-gq %d changes nothing in the table" % q
    return tables


def test_cli_sample_stats_on_the_haploid_cohort(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    _cli(["index"] + COMMON + [fa, vcf, fq])

    def run(opts, group, d, env):
        assert _cli(["call"] + COMMON + opts + group + ["--cohort", "--merged", str(d / "m.vcf"), "-v", "--sample-stats", str(d / "s.tsv"), fa, vcf, man],
                    env=dict(os.environ, **env)) == ""
    tables = _check_cohort(run, [["--cohort-group", "3"], ["--cohort-group", "2"]], tmp_path, diploid=False)
    # -o alone, without --merged: the same table (one group, and groups of 3 + 1)
    for i, group in enumerate(([], ["--cohort-group", "3"])):
        d = tmp_path / ("o%d" % i)
        d.mkdir()
        assert _cli(["call"] + COMMON + group + ["--cohort", "-o", str(d / "out"), "--sample-stats", str(d / "s.tsv"), fa, vcf, man]) == ""
        _no_leftovers(d, ["out", "s.tsv"])
        assert open(str(d / "s.tsv")).read() == tables["all"]
    _no_leftovers(tmp, ["haploid.fq", "dump.txt", "sim1.fq", "sim2.fq", "keep.txt", "cohort.tsv"] + [f for f in os.listdir(tmp) if f.startswith("haploid.vcf.gz")])


def test_cli_sample_stats_on_general_blocks(tmp_path):
    """the diploid panel of tests/test_gpu_pairs.py::test_cli_pairs_on_general_blocks: multi-allelic records, heterozygous cells,
    insertions and deletions; grouped runs in batches of 7 records"""
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

    def run(opts, group, d, env):
        assert _cli(["call", "--cohort", "-v"] + opts + group + ["--merged", str(d / "m.vcf"), "--sample-stats", str(d / "s.tsv")] + common + [str(data / "cohort.tsv")],
                    env=dict(env0, **env)) == ""
    _check_cohort(run, [["--cohort-group", "3"], ["--cohort-group", "2"]], tmp_path, diploid=True)
    merged = open(str(tmp_path / "all" / "m.vcf")).read()
    assert any("," in r.split("\t")[4] for r in _split(merged)[1]), "no multi-allelic record"
    assert not [f for f in os.listdir(data) if f.endswith(".part")]
