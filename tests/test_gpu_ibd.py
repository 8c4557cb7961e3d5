"""`call --cohort --ibd PATH`: IBS0-free segments per pair of samples -- the records' words turned into bit planes in the records' order
(mg_sites_to_planes) and the walk of every pair along them with its state kept on the device (mg_ibd_begin / mg_ibd_step), both made on
the device.

The ABI is compared with the restatement of tests/ibd_model.py over the case table of tests/ibd_cases.py; the command line with that
restatement applied to the merged VCF the same run wrote.  Every value is an integer and every comparison exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ibd_cases
from ibd_model import HEADER, IBD_SEG, IbdModel, ibd_segments, ibd_table_text, sort_segments
from malva_amd import Context, MalvaError, capi
from test_gpu_ld import _cells_case, _dev

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE, MG_ERR_LIMIT = -1, -3, -5
MIN_GQ = 30
POISON = 0xDEADBEEFDEADBEEF
PAD = 8
FIELDS = ("a", "b", "chrom", "start_pos", "end_pos", "n", "ibs2", "zero")


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def _same(got, want):
    """two IBD_SEG arrays, field by field"""
    assert got.dtype == IBD_SEG and len(got) == len(want), (len(got), len(want))
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), f


def test_the_struct_is_the_models():
    assert capi.IBD_SEG == IBD_SEG and IBD_SEG.itemsize == 32 and capi.IBD_MAX_SAMPLES == 16384


# ---- the ABI: the transpose ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4097])
@pytest.mark.parametrize("planes", [1, 64, 65, 130])
def test_transpose_equals_pack_dosage(ctx, planes, n):
    """the groups' mg_pack_site_dosage outputs, transposed, are mg_pack_dosage of the same cells, bit for bit"""
    g1, g2, gq, vao = _cells_case(planes, n, seed=planes * 10000 + n)
    groups = [(s, min(64, planes - s)) for s in range(0, planes, 64)]
    G, W = len(groups), (n + 63) // 64
    sites = np.stack([ctx.pack_site_dosage(g1[s:s + k], g2[s:s + k], gq[s:s + k], False, vao, min_gq=MIN_GQ) for s, k in groups])
    want = np.zeros((64 * G, 3, W), dtype=np.uint64)
    for g, (s, k) in enumerate(groups):
        want[64 * g:64 * g + k] = ctx.pack_dosage(g1[s:s + k], g2[s:s + k], gq[s:s + k], False, vao, min_gq=MIN_GQ)
    if n >= 63:
        assert all(want[:planes, d].any() for d in range(3))
    got = ctx.sites_to_planes(sites, out=np.full((64 * G, 3, W), POISON, dtype=np.uint64))
    assert np.array_equal(got, want), "host form"
    if n % 64:
        assert not (got[:, :, -1] >> np.uint64(n % 64)).any(), "bits at and beyond n_vars"
    # the device form into a poisoned buffer between guard words: every word is written, nothing beyond
    words = 64 * G * 3 * W
    ds = _dev(sites)
    out = _dev(np.full(words + 2 * PAD, POISON, dtype=np.uint64))
    torch.cuda.synchronize()
    ctx.sites_to_planes_device(n, G, ds.data_ptr(), out.data_ptr() + 8 * PAD)
    ctx.synchronize()
    h = out.cpu().numpy().view(np.uint64)
    assert (h[:PAD] == POISON).all() and (h[PAD + words:] == POISON).all(), "written outside the planes"
    assert np.array_equal(h[PAD:PAD + words].reshape(64 * G, 3, W), want), "device form"


# ---- the ABI: the steps against the model ------------------------------------------------------------------------------------------------

def _walk(ctx, case, cuts, cap=None):
    """the case through mg_ibd_begin and one mg_ibd_step per piece of `cuts`, the last one flushing -> the steps' outputs sorted"""
    n = case["D"].shape[0]
    ctx.ibd_begin(case["n_samples"], case["min_records"], case["min_bp"])
    edges = [0] + list(cuts) + [n]
    parts = []
    for i, (c0, c1) in enumerate(zip(edges[:-1], edges[1:])):
        seg = ctx.ibd_step(case["words"][:, :, c0:c1], case["chrom"][c0:c1], case["pos"][c0:c1], flush=i == len(edges) - 2, segs_cap=cap)
        key = seg["a"].astype(np.int64) << 32 | seg["b"].astype(np.int64)
        assert (np.diff(key) >= 0).all(), "a step's segments are ordered by (a, b)"
        parts.append(seg.copy())
    ctx.ibd_end()
    return sort_segments(parts)


CASES = ibd_cases.directed_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_steps_on_a_directed_case(ctx, case):
    want = ibd_segments(case["D"], case["chrom"], case["pos"], case["n_samples"], case["min_records"], case["min_bp"])
    if case["expect"] is not None:
        assert len(want) == len(case["expect"])
    for cuts in case["cuts"]:
        _same(_walk(ctx, case, cuts), want)


@pytest.fixture(scope="module")
def random_cases():
    """the random cases with the model's table, made once and left unchanged"""
    made = {}

    def get(key):
        if key not in made:
            c = ibd_cases.random_case(*key)
            m = IbdModel(c["n_samples"], c["min_records"], c["min_bp"])
            want = ibd_segments(c["D"], c["chrom"], c["pos"], c["n_samples"], 0, 0, model=m)
            want.setflags(write=False)
            made[key] = (c, want, dict(m.filtered))
        return made[key]
    return get


@pytest.mark.parametrize("key", ibd_cases.RANDOM, ids=["%d-%d-%d" % k[:3] for k in ibd_cases.RANDOM])
def test_steps_on_a_random_case(ctx, random_cases, key):
    case, want, filtered = random_cases(key)
    assert len(want) >= 1 and filtered["min_bp"] >= 1
    assert filtered["min_records"] >= 1 or case["min_records"] == 1     # (every closed run has n >= 1: min_records 1 cannot filter)
    for cuts in case["cuts"]:
        _same(_walk(ctx, case, cuts), want)


def test_the_device_form_between_guard_words(ctx, random_cases):
    case, want, _ = random_cases(ibd_cases.RANDOM[1])
    n, G = case["D"].shape[0], case["words"].shape[0]
    k = len(want)
    ds, dc, dp = _dev(case["words"]), _dev(case["chrom"]), _dev(case["pos"])
    out = _dev(np.full(4 * (k + 2 * PAD), POISON, dtype=np.uint64))
    torch.cuda.synchronize()
    ctx.ibd_begin(case["n_samples"], case["min_records"], case["min_bp"])
    rc, need = ctx.ibd_step_device(n, G, ds.data_ptr(), dc.data_ptr(), dp.data_ptr(), True, out.data_ptr() + 32 * PAD, k)
    ctx.synchronize()
    ctx.ibd_end()
    h = out.cpu().numpy().view(np.uint64)
    assert (rc, need) == (0, k)
    assert (h[:4 * PAD] == POISON).all() and (h[4 * (PAD + k):] == POISON).all(), "written outside the segments' buffer"
    _same(h[4 * PAD:4 * (PAD + k)].copy().view(IBD_SEG), want)


# ---- the ABI: the LIMIT contract -----------------------------------------------------------------------------------------------------

def test_a_buffer_too_small_does_not_advance_the_state(ctx, random_cases):
    case, want, _ = random_cases(ibd_cases.RANDOM[1])
    n = case["D"].shape[0]
    cuts = [0, n // 3, 2 * n // 3, n]
    ctx.ibd_begin(case["n_samples"], case["min_records"], case["min_bp"])
    parts, refused = [], 0
    for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
        args = (case["words"][:, :, c0:c1], case["chrom"][c0:c1], case["pos"][c0:c1])
        flush = i == 2
        # what the step needs, from the model cut the same way
        m = IbdModel(case["n_samples"], case["min_records"], case["min_bp"])
        for j in range(i):
            m.step(case["D"][cuts[j]:cuts[j + 1]], case["chrom"][cuts[j]:cuts[j + 1]], case["pos"][cuts[j]:cuts[j + 1]])
        need = len(m.step(case["D"][c0:c1], case["chrom"][c0:c1], case["pos"][c0:c1], flush=flush))
        assert need > 1
        for cap in (need - 1, 0, need // 2):                                       # refused, again and again: nothing moves
            buf = np.full(4 * max(cap, 1), POISON, dtype=np.uint64).view(IBD_SEG)
            with pytest.raises(MalvaError) as e:
                ctx.ibd_step(*args, flush=flush, segs_cap=cap, segs=buf)
            assert e.value.code == MG_ERR_LIMIT and e.value.needed == need, "the exact need is reported"
            assert (buf.view(np.uint64) == POISON).all(), "nothing is written to segs_out"
            refused += 1
        buf = np.full(4 * (need + PAD), POISON, dtype=np.uint64).view(IBD_SEG)
        seg = ctx.ibd_step(*args, flush=flush, segs_cap=need, segs=buf)             # the same call with enough room
        assert len(seg) == need and (buf.view(np.uint64)[4 * need:] == POISON).all()
        parts.append(seg.copy())
    ctx.ibd_end()
    assert refused == 9
    _same(sort_segments(parts), want)


# ---- the ABI: arguments, state, stats ------------------------------------------------------------------------------------------------

def test_argument_and_state_errors():
    case = next(c for c in CASES if c["name"] == "samples_65")
    words, chrom, pos = (np.ascontiguousarray(case[k]) for k in ("words", "chrom", "pos"))
    n = words.shape[2]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with Context(35, 43, 1 << 20) as c:
        L, h = c._L, c.h
        segs, need = np.zeros(1 << 17, dtype=IBD_SEG), C.c_uint64(77)
        planes = np.zeros((128, 3, (n + 63) // 64), dtype=np.uint64)
        for form in (L.mg_sites_to_planes, L.mg_sites_to_planes_device):
            assert form(h, n, 0, p(words), p(planes)) == MG_ERR_ARG
            assert form(h, n, capi.LD_MAX_GROUPS + 1, p(words), p(planes)) == MG_ERR_ARG
            assert form(h, n, 2, None, p(planes)) == MG_ERR_ARG
            assert form(h, n, 2, p(words), None) == MG_ERR_ARG
            assert form(None, n, 2, p(words), p(planes)) == MG_ERR_ARG
            assert form(h, 0, 2, None, None) == 0                                   # no records: nothing to write
        assert not planes.any()
        ok = dict(n_vars=n, n_groups=2, sites=p(words), chrom=p(chrom), pos=p(pos), flush=1, segs=p(segs), cap=1 << 17, need=C.byref(need))
        for form in (L.mg_ibd_step, L.mg_ibd_step_device):
            assert form(h, *ok.values()) == MG_ERR_STATE, "a step without begin"
        assert L.mg_ibd_end(h) == 0, "an end without begin is legal"
        for bad in ((1, 1, 0), (capi.IBD_MAX_SAMPLES + 1, 1, 0), (65, 0, 0), (65, 1, 1 << 63)):
            assert L.mg_ibd_begin(h, *bad) == MG_ERR_ARG, bad
        assert L.mg_ibd_begin(None, 65, 1, 0) == MG_ERR_ARG
        for form in (L.mg_ibd_step, L.mg_ibd_step_device):
            assert form(h, *ok.values()) == MG_ERR_STATE, "a refused begin leaves no state"
        assert L.mg_ibd_begin(h, 65, 3, 0) == 0
        for form in (L.mg_ibd_step, L.mg_ibd_step_device):
            for change in (dict(n_groups=1), dict(n_groups=3), dict(sites=None), dict(chrom=None), dict(pos=None), dict(need=None), dict(segs=None)):
                assert form(h, *dict(ok, **change).values()) == MG_ERR_ARG, change
            assert form(None, *ok.values()) == MG_ERR_ARG
        assert not segs.view(np.uint8).any() and need.value == 77, "an argument error writes nothing"
        assert L.mg_ibd_step(h, *dict(ok, n_vars=0, sites=None, chrom=None, pos=None, flush=0, segs=None, cap=0).values()) == 0 and need.value == 0
        assert L.mg_ibd_step(h, *ok.values()) == 0
        want = ibd_segments(case["D"], chrom, pos, 65, 3, 0)
        _same(segs[:need.value], want)
        assert L.mg_ibd_step(h, *dict(ok, n_vars=0, sites=None, chrom=None, pos=None, flush=1, segs=None, cap=0).values()) == 0 and need.value == 0, "nothing is open"
        assert L.mg_ibd_end(h) == 0
        assert L.mg_ibd_step(h, *ok.values()) == MG_ERR_STATE, "a step behind the end"
        assert L.mg_ibd_stats(h, None) == MG_ERR_ARG


def test_begin_end_begin_again(ctx):
    """a second begin discards the first, open runs included; so does an end"""
    case = next(c for c in CASES if c["name"] == "run_across_three_chunks")
    args = lambda c0, c1: (case["words"][:, :, c0:c1], case["chrom"][c0:c1], case["pos"][c0:c1])
    want = ibd_segments(case["D"][100:], case["chrom"][100:], case["pos"][100:], 2, 1, 0)
    assert len(want) == 1 and want[0]["n"] == 100
    ctx.ibd_begin(2, 1, 0)
    assert len(ctx.ibd_step(*args(0, 100))) == 0                                    # the run stays open ...
    ctx.ibd_begin(2, 1, 0)                                                          # ... and is forgotten
    _same(ctx.ibd_step(*args(100, 200), flush=True), want)
    ctx.ibd_begin(2, 1, 0)
    assert len(ctx.ibd_step(*args(0, 100))) == 0
    ctx.ibd_end()
    ctx.ibd_begin(130, 50, 0)                                                       # another size, other thresholds
    big = next(c for c in CASES if c["name"] == "samples_130")
    long_runs = ibd_segments(big["D"], big["chrom"], big["pos"], 130, 50, 0)
    assert 0 < len(long_runs) < 8385 and (long_runs["n"] >= 50).all()
    _same(ctx.ibd_step(big["words"], big["chrom"], big["pos"], flush=True), long_runs)
    ctx.ibd_begin(2, 1, 0)
    _same(ctx.ibd_step(*args(100, 200), flush=True), want)
    ctx.ibd_end()


def test_ibd_stats_before_and_after():
    case = next(c for c in CASES if c["name"] == "samples_64")
    with Context(35, 43, 1 << 20) as c:
        ms = (C.c_float * 2)(5.0, 5.0)
        assert c._L.mg_ibd_stats(c.h, ms) == MG_ERR_STATE and tuple(ms) == (0.0, 0.0)
        c.sites_to_planes(case["words"])
        first = c.ibd_stats()
        assert first[0] > 0 and first[1] == 0, "no step yet"
        c.ibd_begin(64, 3, 0)
        c.ibd_step(case["words"], case["chrom"], case["pos"], flush=True)
        ms = c.ibd_stats()
        assert ms[0] > 0 and ms[1] >= ms[0], "the step's time holds its own transpose"
        c.pack_dosage(np.zeros((2, 5), dtype=np.int32), np.zeros((2, 5), dtype=np.int32), None, False, np.arange(0, 12, 2, dtype=np.uint32))
        assert c.ibd_stats() == ms, "a neighbour changed mg_ibd_stats"
        c.ibd_end()
        assert c.ibd_stats() == ms


# ---- the command line -------------------------------------------------------------------------------------------------------------

from test_gpu_merged import BIN, COMMON, _cli, _no_leftovers, haploid_cohort  # noqa: E402,F401 (the fixture)
from test_gpu_site_tags import _median_gq  # noqa: E402

IBD_OPTS = ["--ibd-min-records", "3", "--ibd-min-bp", "0"]


def _rows(table):
    lines = table.split("\n")
    assert lines[-1] == "" and lines[0] + "\n" == HEADER
    return [l.split("\t") for l in lines[1:-1]]


def _check_ibd_cohort(run, groups, tmp_path):
    """run(opts, group, directory, env, ibd, ld) writes directory/m.vcf and, as asked, directory/ibd.tsv and directory/ld.tsv; groups: the grouped
    runs that must give the same bytes.  The expected table is the model applied to the merged VCF the same run wrote."""
    tables = {}
    q = None
    for tag in ("all", "masked"):
        opts = IBD_OPTS + ([] if q is None else ["--min-gq", str(q)])
        d = tmp_path / tag
        d.mkdir()
        run(opts, [], d, {}, True, False)
        _no_leftovers(d, ["m.vcf", "ibd.tsv"])
        merged = open(str(d / "m.vcf")).read()
        table = open(str(d / "ibd.tsv")).read()
        assert table == ibd_table_text(merged, min_records=3, min_bp=0, min_gq=q), tag
        tables[tag] = table
        for i, (group, batch) in enumerate(groups if q is None else groups[:1]):   # whatever the grouping, the batches and the chunks: the same bytes
            g = tmp_path / ("%s-g%d" % (tag, i))
            g.mkdir()
            run(opts, group, g, {"MALVA_GENO_BATCH": batch}, True, False)
            _no_leftovers(g, ["m.vcf", "ibd.tsv"])
            assert open(str(g / "ibd.tsv")).read() == table, "%s %s batch %s" % (tag, group, batch)
            assert open(str(g / "m.vcf")).read() == merged
        if q is None:
            both, ld_alone = tmp_path / "both", tmp_path / "ld"                     # with --ld as well, and --ld without --ibd: every other output the same bytes
            both.mkdir(), ld_alone.mkdir()
            run(IBD_OPTS, ["--cohort-group", "2"], both, {"MALVA_GENO_BATCH": "7"}, True, True)
            run([], ["--cohort-group", "2"], ld_alone, {"MALVA_GENO_BATCH": "7"}, False, True)
            _no_leftovers(both, ["m.vcf", "ibd.tsv", "ld.tsv"])
            _no_leftovers(ld_alone, ["m.vcf", "ld.tsv"])
            assert open(str(both / "ibd.tsv")).read() == table
            for f in ("m.vcf", "ld.tsv"):
                assert open(str(both / f)).read() == open(str(ld_alone / f)).read(), f
            assert open(str(both / "m.vcf")).read() == merged and len(open(str(both / "ld.tsv")).read().split("\n")) > 3
            q = _median_gq(merged)
    assert tables["all"] != tables["masked"], "--min-gq %d changes nothing in the table" % q
    return tables


def test_cli_ibd_on_the_haploid_cohort(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    _cli(["index"] + COMMON + [fa, vcf, fq])

    def run(opts, group, d, env, ibd, ld):
        assert _cli(["call"] + COMMON + opts + group + ["--cohort", "--merged", str(d / "m.vcf")] + (["--ibd", str(d / "ibd.tsv")] if ibd else []) +
                    (["--ld", str(d / "ld.tsv")] if ld else []) + [fa, vcf, man], env=dict(os.environ, **env)) == ""
    tables = _check_ibd_cohort(run, [(["--cohort-group", "2"], "3"), (["--cohort-group", "3"], "7"), ([], "3")], tmp_path)
    rows = _rows(tables["all"])
    assert len(rows) >= 5 and all(int(r[6]) >= 3 and int(r[5]) == int(r[4]) - int(r[3]) and int(r[7]) <= int(r[6]) for r in rows)
    # the defaults (100 records, 1 Mb), and -o alone, without --merged: one group, and groups of 3 + 1
    merged = open(str(tmp_path / "all" / "m.vcf")).read()
    want = ibd_table_text(merged)
    for i, group in enumerate(([], ["--cohort-group", "3"])):
        d = tmp_path / ("o%d" % i)
        d.mkdir()
        assert _cli(["call"] + COMMON + group + ["--cohort", "-o", str(d / "out"), "--ibd", str(d / "ibd.tsv"), fa, vcf, man]) == ""
        _no_leftovers(d, ["out", "ibd.tsv"])
        assert open(str(d / "ibd.tsv")).read() == want
    d = tmp_path / "bp"                                                            # the other threshold
    d.mkdir()
    assert _cli(["call"] + COMMON + ["--cohort", "--merged", str(d / "m.vcf"), "--ibd", str(d / "ibd.tsv"), "--ibd-min-records", "1", "--ibd-min-bp", "300", fa, vcf, man]) == ""
    got = open(str(d / "ibd.tsv")).read()
    assert got == ibd_table_text(merged, min_records=1, min_bp=300) and all(int(r[5]) >= 300 for r in _rows(got))
    _no_leftovers(tmp, ["haploid.fq", "dump.txt", "sim1.fq", "sim2.fq", "keep.txt", "cohort.tsv"] + [f for f in os.listdir(tmp) if f.startswith("haploid.vcf.gz")])


def test_cli_ibd_on_general_blocks(tmp_path):
    """the diploid panel of tests/test_gpu_ld.py::test_cli_ld_on_general_blocks: multi-allelic records (NEUT) and heterozygous cells; grouped runs
    in batches and chunks of 7 records"""
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

    def run(opts, group, d, env, ibd, ld):
        assert _cli(["call", "--cohort"] + opts + group + ["--merged", str(d / "m.vcf")] + (["--ibd", str(d / "ibd.tsv")] if ibd else []) +
                    (["--ld", str(d / "ld.tsv")] if ld else []) + common + [str(data / "cohort.tsv")], env=dict(env0, **env)) == ""
    tables = _check_ibd_cohort(run, [(["--cohort-group", "2"], "7"), ([], "7"), (["--cohort-group", "2"], "400")], tmp_path)
    rows = _rows(tables["all"])
    assert len(rows) > 10 and {(r[0], r[1]) for r in rows} == {("s0", "s1"), ("s0", "s2"), ("s1", "s2")} and any(r[7] != r[6] for r in rows)
    assert rows == sorted(rows, key=lambda r: (r[0], r[1])), "ordered by pair"
    assert not [f for f in os.listdir(data) if f.endswith(".part")]


def test_cli_ibd_usage_errors_write_nothing(haploid_cohort, tmp_path):
    import subprocess
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    ibd = str(tmp_path / "ibd.tsv")
    base = ["call"] + COMMON + ["--cohort", "--merged", str(tmp_path / "m.vcf")]
    bad = [base + ["--ibd-min-records", "5"],                                      # a sub-option without --ibd
           base + ["--ibd-min-bp", "5"],
           base + ["--ibd", ibd, "--ibd-min-records", "0"], base + ["--ibd", ibd, "--ibd-min-records", "4294967296"], base + ["--ibd", ibd, "--ibd-min-records", "x"],
           base + ["--ibd", ibd, "--ibd-min-records", "-3"], base + ["--ibd", ibd, "--ibd-min-bp", "-1"], base + ["--ibd", ibd, "--ibd-min-bp", "1e6"],
           base + ["--ibd", ""],
           ["call"] + COMMON + ["--ibd", ibd]]                                     # without --cohort
    for args in bad:
        r = subprocess.run([BIN] + args + [fa, vcf, man if "--cohort" in args else fq], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "malva : --ibd" in r.stderr and r.stdout == "", args
        assert not os.listdir(tmp_path), args
    r = subprocess.run([BIN] + base + ["--ibd-min-bp", "5", fa, vcf, man], capture_output=True, text=True, timeout=120)
    assert "--ibd-min-records and --ibd-min-bp go with --ibd" in r.stderr
    r = subprocess.run([BIN, "call"] + COMMON + ["--ibd", ibd, fa, vcf, fq], capture_output=True, text=True, timeout=120)
    assert "--ibd goes with --cohort" in r.stderr
