"""`call --cohort --pairs PATH`: the table of pairwise genotype sharing, packed and counted on the device (mg_pack_dosage,
mg_pair_counts).

The ABI is compared with the numpy restatement of tests/test_pairs_cpu.py; the command line with that restatement applied to the
merged VCF the same run wrote -- the project's own published output, not its internals.  Every comparison is exact: the results
are integers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from malva_amd import Context, MalvaError, synth
from test_gpu_merged import COMMON, _case, _cli, _no_leftovers, _split, format_plain, haploid_cohort  # noqa: F401 (the fixture)
from test_gpu_site_tags import _median_gq, counts_numpy
from test_pairs_cpu import pack_plain, pair_plain, pairs_text

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE = -1, -3
ONES = np.uint64((1 << 64) - 1)
MIN_GQ = 30


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


# ---- the ABI: packing -----------------------------------------------------------------------------------------------------------

def _cells_case(planes, n, seed):
    """records of 1, 2 and 3 alleles (mostly 2), allele indexes 0 and 1 with -1 and 2 strewn over every kind of record, gq on both
    sides of MIN_GQ"""
    rng = np.random.default_rng(seed)
    A = rng.choice(np.array([1, 2, 2, 2, 2, 3]), size=n)
    if n >= 3:
        A[:3] = (2, 1, 3)
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)

    def draw():
        g = rng.integers(0, 2, size=(planes, n))
        stray = rng.random((planes, n)) < 0.06
        g[stray] = rng.choice(np.array([-1, 2]), size=int(stray.sum()))
        return g.astype(np.int32)
    return draw(), draw(), rng.integers(0, 2 * MIN_GQ, size=(planes, n)).astype(np.int32), vao


@pytest.fixture(scope="module")
def pack_cases():
    """cells and their packed form by numpy, made once per (planes, n, haploid, masked)"""
    made = {}

    def get(planes, n, haploid, masked):
        key = (planes, n, haploid, masked)
        if key not in made:
            cells = made.get(("cells", planes, n))
            if cells is None:
                cells = made[("cells", planes, n)] = _cells_case(planes, n, seed=planes * 1000 + n % 997)
            g1, g2, gq, vao = cells
            want = pack_plain(g1, g2, gq, haploid, vao, MIN_GQ if masked else None)
            want.setflags(write=False)
            made[key] = cells + (want,)
        return made[key]
    return get


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100003])
@pytest.mark.parametrize("masked", [False, True], ids=["all-called", "masked"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 3, 17, 64])
def test_pack_is_exact(ctx, pack_cases, planes, haploid, masked, n):
    g1, g2, gq, vao, want = pack_cases(planes, n, haploid, masked)
    W = (n + 63) // 64
    if n >= 257:                                                                   # the case has what it is meant to have
        A = np.diff(vao.astype(np.int64))
        two = np.broadcast_to(A == 2, g1.shape)
        assert all((A == a).any() for a in (1, 2, 3)) and (g1[two] == -1).any() and (g1[two] == 2).any()
        assert (gq < MIN_GQ).any() and (gq >= MIN_GQ).any()
        assert want[:, 0].any() and want[:, 2].any() and want[:, 1].any() != haploid
        assert not masked or not np.array_equal(want, pack_plain(g1, g2, gq, haploid, vao, None))
    out = np.full((planes, 3, W), ONES, dtype=np.uint64)                           # a buffer of ones comes back fully overwritten
    got = ctx.pack_dosage(g1, None if haploid else g2, gq if masked else None, haploid, vao, min_gq=MIN_GQ if masked else None, out=out)
    assert got is out and np.array_equal(got, want)
    if n % 64:
        assert not (got[:, :, -1] >> np.uint64(n % 64)).any(), "bits at and beyond n_vars are set"
    assert not (got[:, 0] & got[:, 1]).any() and not (got[:, 0] & got[:, 2]).any() and not (got[:, 1] & got[:, 2]).any(), "a cell has two bits set"
    ms = ctx.pairs_stats()
    assert len(ms) == 2 and all(np.isfinite(m) and m >= 0 for m in ms)


# ---- the ABI: counting ----------------------------------------------------------------------------------------------------------

def _words_case(n, n_words, seed):
    """planes of several densities: all ones, a half, an eighth, none -- dealt out row by row"""
    rng = np.random.default_rng(seed)
    r = lambda: rng.integers(0, 1 << 64, size=(n, 3, n_words), dtype=np.uint64)
    w = r()
    kind = rng.integers(0, 4, size=(n, 3))
    kind.flat[:min(4, kind.size)] = (0, 1, 2, 3)[:kind.size]
    w[kind == 0] = ONES
    w[kind == 2] &= (r() & r())[kind == 2]
    w[kind == 3] = 0
    return w


@pytest.fixture(scope="module")
def count_cases():
    """words and their counts by numpy, made once per (n_a, n_b, n_words) and left unchanged"""
    made = {}

    def get(n_a, n_b, n_words):
        key = (n_a, n_b, n_words)
        if key not in made:
            a, b = _words_case(n_a, n_words, seed=n_a * 100 + n_words), _words_case(n_b, n_words, seed=n_b * 100 + n_words + 7)
            made[key] = (a, b, pair_plain(a, b), pair_plain(a))
            for x in made[key]:
                x.setflags(write=False)
        return made[key]
    return get


@pytest.mark.parametrize("n_words", [0, 1, 2, 33, 1563])
@pytest.mark.parametrize("n_a,n_b", [(1, 1), (3, 5), (17, 17), (64, 64), (64, 1)])
def test_count_is_exact(ctx, count_cases, n_a, n_b, n_words):
    a, b, want, want_self = count_cases(n_a, n_b, n_words)
    if n_words:
        assert want.any() and int(want.max()) == 64 * n_words                      # (two rows of ones meet somewhere, or the case is too thin)
    garbage = np.full((n_a, n_b, 3, 3), np.uint64(0xDEADBEEFDEADBEEF), dtype=np.uint64)
    got = ctx.pair_counts(a, b, counts=garbage, overwrite=True)                    # accumulate == 0 over garbage overwrites it
    assert got is garbage and np.array_equal(got, want)
    # B == NULL: the square, equal to the explicit form and symmetric
    square = ctx.pair_counts(a)
    assert np.array_equal(square, want_self)
    assert np.array_equal(square, ctx.pair_counts(a, a))
    assert np.array_equal(square, square.transpose(1, 0, 3, 2))
    # the words cut at an arbitrary point and counted in two calls
    cut = (n_words * 5) // 13
    two = ctx.pair_counts(a[:, :, :cut], b[:, :, :cut])
    assert ctx.pair_counts(a[:, :, cut:], b[:, :, cut:], counts=two) is two
    assert np.array_equal(two, want)
    two = ctx.pair_counts(a[:, :, :cut])
    ctx.pair_counts(a[:, :, cut:], counts=two)
    assert np.array_equal(two, want_self)
    ms = ctx.pairs_stats()
    assert len(ms) == 2 and all(np.isfinite(m) and m >= 0 for m in ms)


@pytest.mark.parametrize("n_words", [1, 33, 1563])
def test_count_of_split_planes_is_the_square(ctx, count_cases, n_words):
    """64 = 40 + 24: four block calls, the two on the diagonal with B == NULL, fill the square"""
    a, _, _, want = count_cases(64, 64, n_words)
    lo, hi = a[:40], a[40:]
    got = np.zeros((64, 64, 3, 3), dtype=np.uint64)
    got[:40, :40] = ctx.pair_counts(lo)
    got[40:, 40:] = ctx.pair_counts(hi)
    got[:40, 40:] = ctx.pair_counts(lo, hi)
    got[40:, :40] = ctx.pair_counts(hi, lo)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:40, 40:], got[40:, :40].transpose(1, 0, 3, 2))


# ---- the ABI: the device forms ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("planes,n", [(3, 257), (17, 100003), (64, 65)])
def test_device_forms_equal_the_host_forms(pack_cases, planes, n):
    """on torch tensors, the context on a stream that is not the default one"""
    g1, g2, gq, vao, want = pack_cases(planes, n, False, True)
    W = (n + 63) // 64
    dev = torch.device("cuda", 0)
    v = C.c_void_p
    with Context(35, 43, 1 << 20) as c:
        side = torch.cuda.Stream(device=dev)
        c.set_stream(side.cuda_stream)
        d1, d2, dq, dv = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (g1, g2, gq, vao))
        guard = 64
        planes_out = torch.full((guard + planes * 3 * W + guard,), -1, dtype=torch.int64, device=dev)
        counts = torch.full((guard + planes * planes * 9 + guard,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        cross = torch.full((planes * 2 * 9,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        d_planes, d_counts = planes_out.data_ptr() + 8 * guard, counts.data_ptr() + 8 * guard
        c._ck(c._L.mg_pack_dosage_device(c.h, n, planes, 0, v(d1.data_ptr()), v(d2.data_ptr()), v(dq.data_ptr()), 1, MIN_GQ, v(dv.data_ptr()), v(d_planes)))
        c._ck(c._L.mg_pair_counts_device(c.h, W, v(d_planes), planes, None, planes, 0, v(d_counts)))
        # the first two planes as B, in two accumulating halves (B's rows are [3][W] apart as A's are)
        if planes > 2:
            c._ck(c._L.mg_pair_counts_device(c.h, W, v(d_planes), planes, v(d_planes), 2, 0, v(cross.data_ptr())))
            c._ck(c._L.mg_pair_counts_device(c.h, W, v(d_planes), planes, v(d_planes), 2, 1, v(cross.data_ptr())))
        c.synchronize()
        hp, hc = planes_out.cpu().numpy(), counts.cpu().numpy()
        for h in (hp, hc):
            assert (h[:guard] == h[0]).all() and (h[-guard:] == h[0]).all(), "words outside the output were written"
        got = hp[guard:-guard].view(np.uint64).reshape(planes, 3, W)
        assert np.array_equal(got, want)
        assert np.array_equal(got, c.pack_dosage(g1, g2, gq, False, vao, min_gq=MIN_GQ))
        host = c.pair_counts(want)
        assert np.array_equal(hc[guard:-guard].view(np.uint64).reshape(planes, planes, 3, 3), host)
        assert np.array_equal(host, pair_plain(want))
        if planes > 2:
            assert np.array_equal(cross.cpu().numpy().view(np.uint64).reshape(planes, 2, 3, 3), 2 * host[:, :2])


# ---- the ABI: arguments, the timer, the neighbours -----------------------------------------------------------------------------------

def test_arguments(ctx):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    g = np.zeros((65, 2), dtype=np.int32)
    vao = np.array([0, 2, 4], dtype=np.uint32)
    out = np.zeros((65, 3, 1), dtype=np.uint64)
    for planes in (0, 65):
        assert ctx._L.mg_pack_dosage(ctx.h, 2, planes, 0, p(g), p(g), p(g), 0, 0, p(vao), p(out)) == MG_ERR_ARG
    assert ctx._L.mg_pack_dosage(ctx.h, 2, 3, 0, p(g), p(g), p(g), 0, 0, None, p(out)) == MG_ERR_ARG     # var_allele_off is required
    assert ctx._L.mg_pack_dosage(ctx.h, 2, 3, 0, p(g), None, p(g), 0, 0, p(vao), p(out)) == MG_ERR_ARG   # diploid: gt2 is read
    assert ctx._L.mg_pack_dosage(ctx.h, 2, 3, 1, p(g), None, None, 0, 0, p(vao), p(out)) == 0            # haploid, no mask: neither is
    with pytest.raises(MalvaError, match="n_planes"):
        ctx.pack_dosage(g, g, g, False, vao)
    words = np.zeros((65, 3, 2), dtype=np.uint64)
    counts = np.zeros(65 * 65 * 9, dtype=np.uint64)
    for n_a, n_b in ((0, 1), (65, 1), (1, 0), (1, 65)):
        assert ctx._L.mg_pair_counts(ctx.h, 2, p(words), n_a, p(words), n_b, 0, p(counts)) == MG_ERR_ARG
    assert ctx._L.mg_pair_counts(ctx.h, 2, p(words), 3, None, 4, 0, p(counts)) == MG_ERR_ARG             # B is A: n_b must be n_a
    assert ctx._L.mg_pair_counts(ctx.h, 2, None, 3, None, 3, 0, p(counts)) == MG_ERR_ARG
    assert ctx._L.mg_pair_counts(ctx.h, 2, p(words), 3, None, 3, 0, None) == MG_ERR_ARG
    counts[:] = 7
    assert ctx._L.mg_pair_counts(ctx.h, 0, None, 3, None, 3, 0, p(counts)) == 0                          # no words: the entries are zeroed
    assert not counts[:81].any() and (counts[81:] == 7).all()


def test_pairs_stats_before_the_first_call_and_with_one_kind_run():
    g1, g2, gq, vao = _cells_case(3, 65, seed=4)
    with Context(35, 43, 1 << 20) as c:
        ms = (C.c_float * 2)(5.0, 5.0)
        assert c._L.mg_pairs_stats(c.h, ms) == MG_ERR_STATE
        with pytest.raises(MalvaError) as e:
            c.pairs_stats()
        assert e.value.code == MG_ERR_STATE
        planes = c.pack_dosage(g1, g2, gq, False, vao)
        ms = c.pairs_stats()
        assert ms[0] >= 0 and ms[1] == 0                                          # 0 for the kind that has not run
        c.pair_counts(planes)
        assert all(np.isfinite(m) and m >= 0 for m in c.pairs_stats())
    with Context(35, 43, 1 << 20) as c:
        c.pair_counts(np.zeros((2, 3, 0), dtype=np.uint64))                        # no words: the call still counts as one
        ms = c.pairs_stats()
        assert ms[0] == 0 and ms[1] >= 0


def test_the_pair_calls_and_their_neighbours_do_not_disturb_each_other():
    """one context: pack, site counts, count, text, pack and count again -- every result what it is alone, the timers of each kind valid"""
    planes, n = 3, 330
    g1, g2, gq, vao = _cells_case(planes, n, seed=12)
    want_planes = pack_plain(g1, g2, gq, False, vao, MIN_GQ)
    want_counts = pair_plain(want_planes)
    want_ac, want_ns = counts_numpy(g1, g2, gq, False, vao, MIN_GQ)
    want_text = format_plain(g1, g2, gq, False)
    with Context(35, 43, 1 << 20) as c:
        packed = c.pack_dosage(g1, g2, gq, False, vao, min_gq=MIN_GQ)
        ac, ns = c.site_counts(g1, g2, gq, False, vao, min_gq=MIN_GQ)
        counts = c.pair_counts(packed)
        text, off = c.format_calls(g1, g2, gq, False)
        again = c.pack_dosage(g1, g2, gq, False, vao, min_gq=MIN_GQ)
        ac2, ns2 = c.site_counts(g1, g2, gq, False, vao, min_gq=MIN_GQ)
        c.pair_counts(again, counts=counts)
        text2, off2 = c.format_calls(g1, g2, gq, False)
        assert np.array_equal(packed, want_planes) and np.array_equal(again, want_planes)
        assert np.array_equal(counts, 2 * want_counts)
        for a, s in ((ac, ns), (ac2, ns2)):
            assert np.array_equal(a, want_ac) and np.array_equal(s, want_ns)
        for t, o in ((text, off), (text2, off2)):
            assert t == want_text[0] and np.array_equal(o, want_text[1])
        assert all(m >= 0 for m in c.pairs_stats() + c.site_stats() + c.format_stats())


# ---- the command line -------------------------------------------------------------------------------------------------------------

def counts_from_vcf(text):
    """-> (names, counts [S, S, 3, 3], called [S]) from a merged VCF: the biallelic records, the cells whose GT is not missing"""
    head, recs = _split(text)
    names = head[-1].split("\t")[9:]
    d = np.full((len(names), len(recs)), -1, dtype=np.int64)
    for v, rec in enumerate(recs):
        cols = rec.split("\t")
        assert cols[8].split(":")[0] == "GT"
        if cols[4] == "." or "," in cols[4]:
            continue
        for s, cell in enumerate(cols[9:]):
            gt = cell.split(":")[0]
            if "." in gt:
                continue
            al = [int(a) for a in gt.split("/")]
            assert all(a in (0, 1) for a in al)
            d[s, v] = sum(al) if len(al) == 2 else 2 * al[0]
    counts = np.zeros((len(names), len(names), 3, 3), dtype=np.uint64)
    for i in range(len(names)):
        for j in range(len(names)):
            both = (d[i] >= 0) & (d[j] >= 0)
            np.add.at(counts[i, j], (d[i][both], d[j][both]), 1)
    return names, counts, (d >= 0).sum(axis=1)


def _table_rows(text):
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0].startswith("#A\tB\tN\t")
    return [l.split("\t") for l in lines[1:-1]]


def _check_cohort(run, groups, tmp_path, diploid):
    """run(opts, group, directory, env) writes directory/m.vcf and directory/p.tsv; groups: the grouped runs that must give the same table"""
    tables = {}
    q = None
    for tag in ("all", "masked"):
        opts = [] if q is None else ["--min-gq", str(q)]
        d = tmp_path / tag
        d.mkdir()
        run(opts, [], d, {})
        _no_leftovers(d, ["m.vcf", "p.tsv"])
        merged = open(str(d / "m.vcf")).read()
        names, counts, called = counts_from_vcf(merged)
        table = open(str(d / "p.tsv")).read()
        assert table == pairs_text(names, counts), tag
        rows = _table_rows(table)
        assert len(rows) == len(names) * (len(names) - 1) // 2 and any(int(r[2]) > 0 for r in rows)
        if diploid:
            assert any(r[-1] != "." for r in rows) and any(int(r[7]) > 0 for r in rows), "no heterozygote in the cohort"
        else:
            assert all(r[-1] == "." and r[4] == r[6] == r[7] == r[8] == r[10] == "0" for r in rows)
        tables[tag] = table
        for i, group in enumerate(groups):                                         # whatever the grouping and the batches: the same bytes
            g = tmp_path / ("%s-g%d" % (tag, i))
            g.mkdir()
            run(opts, group, g, {"MALVA_GENO_BATCH": "7"})
            _no_leftovers(g, ["m.vcf", "p.tsv"])
            assert open(str(g / "p.tsv")).read() == table, "%s %s" % (tag, group)
            assert open(str(g / "m.vcf")).read() == merged
        if q is None:
            q = _median_gq(merged)
    assert tables["all"] != tables["masked"], "--min-gq %d changes nothing in the table" % q
    return tables


def test_cli_pairs_on_the_haploid_cohort(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    _cli(["index"] + COMMON + [fa, vcf, fq])

    def run(opts, group, d, env):
        assert _cli(["call"] + COMMON + opts + group + ["--cohort", "--merged", str(d / "m.vcf"), "--pairs", str(d / "p.tsv"), fa, vcf, man],
                    env=dict(os.environ, **env)) == ""
    tables = _check_cohort(run, [["--cohort-group", "3"]], tmp_path, diploid=False)
    # -o alone, without --merged: the same table (one group, and groups of 3 + 1)
    for i, group in enumerate(([], ["--cohort-group", "3"])):
        d = tmp_path / ("o%d" % i)
        d.mkdir()
        assert _cli(["call"] + COMMON + group + ["--cohort", "-o", str(d / "out"), "--pairs", str(d / "p.tsv"), fa, vcf, man]) == ""
        _no_leftovers(d, ["out", "p.tsv"])
        assert open(str(d / "p.tsv")).read() == tables["all"]
    # one input under two names: the pair agrees everywhere
    d = tmp_path / "twice"
    d.mkdir()
    (d / "cohort.tsv").write_text("first\t%s\nother\t%s\nsecond\t%s\n" % (fq, str(tmp / "sim1.fq"), fq))
    for i, group in enumerate(([], ["--cohort-group", "2"])):
        out = d / ("g%d" % i)
        out.mkdir()
        assert _cli(["call"] + COMMON + group + ["--cohort", "--merged", str(out / "m.vcf"), "--pairs", str(out / "p.tsv"), fa, vcf, str(d / "cohort.tsv")]) == ""
        _no_leftovers(out, ["m.vcf", "p.tsv"])
        names, counts, called = counts_from_vcf(open(str(out / "m.vcf")).read())
        rows = {(r[0], r[1]): r for r in _table_rows(open(str(out / "p.tsv")).read())}
        assert names == ["first", "other", "second"] and sorted(rows) == [("first", "other"), ("first", "second"), ("other", "second")]
        r = rows[("first", "second")]
        n00, n01, n02, n10, n11, n12, n20, n21, n22 = (int(x) for x in r[3:12])
        assert n01 == n02 == n10 == n12 == n20 == n21 == 0 and int(r[12]) == 0
        assert int(r[2]) == n00 + n11 + n22 == int(called[0]) == int(called[2]) > 0
        assert int(rows[("first", "other")][12]) > 0, "the third sample agrees with the first everywhere: the case shows nothing"
    _no_leftovers(tmp, ["haploid.fq", "dump.txt", "sim1.fq", "sim2.fq", "keep.txt", "cohort.tsv"] + [f for f in os.listdir(tmp) if f.startswith("haploid.vcf.gz")])


def test_cli_pairs_on_general_blocks(tmp_path):
    """the diploid panel of tests/test_gpu_merged.py::test_cli_merged_on_general_blocks: multi-allelic records (left out of the table) and
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

    def run(opts, group, d, env):
        assert _cli(["call", "--cohort"] + opts + group + ["--merged", str(d / "m.vcf"), "--pairs", str(d / "p.tsv")] + common + [str(data / "cohort.tsv")],
                    env=dict(env0, **env)) == ""
    _check_cohort(run, [["--cohort-group", "3"], ["--cohort-group", "2"]], tmp_path, diploid=True)
    merged = open(str(tmp_path / "all" / "m.vcf")).read()
    assert any("," in r.split("\t")[4] for r in _split(merged)[1]), "no multi-allelic record"
    assert not [f for f in os.listdir(data) if f.endswith(".part")]
