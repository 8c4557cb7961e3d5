"""`call --cohort --grm PATH`: the genetic relationship matrix -- the records' weights (mg_grm_weights), their expansion into signed bytes
and the Gram products on the matrix cores with the pairs' sums kept on the device (mg_grm_begin / mg_grm_step / mg_grm_read).

The ABI is compared with the restatement of tests/grm_model.py over the case table of tests/grm_cases.py; the command line with that
restatement applied to the merged VCF the same run wrote.  Every value is an integer and every comparison exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import grm_cases
import grm_model as M
from malva_amd import Context, capi
from test_gpu_ld import _dev

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE = -1, -3
POISON16 = np.int16(0x5A5A)
PAD = 16


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def test_the_constants_are_the_models():
    assert (capi.GRM_MAX_SAMPLES, capi.GRM_SHIFT, capi.GRM_MAX_Q) == (M.MAX_SAMPLES, M.SHIFT, M.MAX_Q) == (16384, 10, 32639)


# ---- the ABI: the weights --------------------------------------------------------------------------------------------------------------

def _words_by_counts(n0, n1, n2, n_samples, seed):
    """records with these counts of dosage 0, 1, 2 -> uint64 [groups, 3, n_vars]: every record's cells at a rotation of its own; the spare
    bits of the last group set"""
    n_vars, G = len(n0), (n_samples + 63) // 64
    rng = np.random.default_rng(seed)
    s = (np.arange(n_samples)[None, :] + rng.integers(0, n_samples, size=(n_vars, 1))) % n_samples      # [v, rank] -> sample
    rank = np.arange(n_samples)[None, :]
    W = np.zeros((G, 3, n_vars), dtype=np.uint64)
    lo = np.zeros(n_vars, dtype=np.int64)
    for d, k in enumerate((n0, n1, n2)):
        hit = (rank >= lo[:, None]) & (rank < (lo + k)[:, None])
        v, r = np.nonzero(hit)
        np.bitwise_or.at(W[:, d, :], (s[v, r] >> 6, v), np.uint64(1) << (s[v, r] & 63).astype(np.uint64))
        lo = lo + k
    if n_samples % 64:
        W[G - 1] |= np.uint64((1 << 64) - (1 << (n_samples % 64)))
    return W


def _check_weights(ctx, W, n_samples, haploid, maf_ppm, min_n, want):
    n = W.shape[2]
    got = ctx.grm_weights(W, n_samples, haploid, maf_ppm, min_n, out=np.full((n, 4), POISON16, dtype=np.int16))
    assert np.array_equal(got, want), "host form: %d records differ" % int((got != want).any(axis=1).sum())
    ds = _dev(W)
    out = _dev(np.full(4 * (n + 2 * PAD), POISON16, dtype=np.int16))
    torch.cuda.synchronize()
    ctx.grm_weights_device(n, W.shape[0], n_samples, ds.data_ptr(), haploid, maf_ppm, min_n, out.data_ptr() + 8 * PAD)
    ctx.synchronize()
    h = out.cpu().numpy().view(np.int16)
    assert (h[:4 * PAD] == POISON16).all() and (h[4 * (PAD + n):] == POISON16).all(), "written outside q_out"
    assert np.array_equal(h[4 * PAD:4 * (PAD + n)].reshape(n, 4), want), "device form"


@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_weights_for_every_count_up_to_40(ctx, haploid):
    t = np.array([(a, b, n - a - b) for n in range(41) for a in range(n + 1) for b in range(n - a + 1)], dtype=np.int64)
    n0, n1, n2 = t[:, 0], t[:, 1], t[:, 2]
    W = _words_by_counts(n0, n1, n2, 40, seed=1)
    for maf_ppm, min_n in ((0, 1), (50000, 7)):
        q, enters = M.weights_from_counts(n0, n1, n2, haploid, maf_ppm, min_n)
        want = np.zeros((len(t), 4), dtype=np.int16)
        want[enters, :3], want[enters, 3] = q[enters], 1
        assert 0 < enters.sum() < len(t)
        _check_weights(ctx, W, 40, haploid, maf_ppm, min_n, want)


@pytest.mark.parametrize("n_samples", [16384, 12345, 509])
@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_weights_for_random_large_counts(ctx, n_samples, haploid):
    rng = np.random.default_rng(n_samples + haploid)
    n_vars = 400
    n = rng.integers(n_samples // 2, n_samples + 1, size=n_vars)
    p = np.where(rng.random(n_vars) < 0.3, rng.uniform(0, 0.004, n_vars), rng.uniform(0, 1, n_vars))   # rare alleles: the |q| limit on both sides
    n2 = rng.binomial(n, p * p)
    n1 = rng.binomial(n - n2, np.minimum(1.0, 2 * p * (1 - p) / np.maximum(1e-12, 1 - p * p)))
    n0 = n - n1 - n2
    W = _words_by_counts(n0, n1, n2, n_samples, seed=2)
    q, enters = M.weights_from_counts(n0, n1, n2, haploid, 1000, 2)
    want = np.zeros((n_vars, 4), dtype=np.int16)
    want[enters, :3], want[enters, 3] = q[enters], 1
    assert 50 < enters.sum() < n_vars - 20
    _check_weights(ctx, W, n_samples, haploid, 1000, 2, want)


def test_weights_of_no_records(ctx):
    assert ctx.grm_weights(np.zeros((2, 3, 0), dtype=np.uint64), 65).shape == (0, 4)


# ---- the ABI: begin / step / read against the model --------------------------------------------------------------------------------------

def _run(ctx, case, words, cuts=(), between=None):
    """begin, one step per piece of `cuts`, read, end -> (S, N, seen, entered)"""
    n = words.shape[2]
    ctx.grm_begin(case["n_samples"], case["haploid"], case["maf_ppm"], case["min_n"])
    edges = [0] + list(cuts) + [n]
    for c0, c1 in zip(edges[:-1], edges[1:]):
        ctx.grm_step(words[:, :, c0:c1])
        if between is not None:
            between(c1)
    out = ctx.grm_read(case["n_samples"])
    ctx.grm_end()
    return out


def _equal(got, want):
    assert got[2:] == want[2:], "records seen, entered"
    assert np.array_equal(got[1], want[1]), "N: %d pairs differ" % int((got[1] != want[1]).sum())
    assert np.array_equal(got[0], want[0]), "S: %d pairs differ" % int((got[0] != want[0]).sum())


def _want(case):
    return M.grm_sums(case["D"], case["n_samples"], case["haploid"], case["maf_ppm"], case["min_n"])


CASES = grm_cases.directed_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_steps_on_a_directed_case(ctx, case):
    words = M.words_from_dosage(case["D"], case["n_samples"])
    want = _want(case)
    if case["enters"] is not None:
        assert want[3] == sum(case["enters"])
    _equal(_run(ctx, case, words), want)
    n = words.shape[2]
    if n > 2:
        _equal(_run(ctx, case, words, cuts=[1, n // 2]), want)


@pytest.fixture(scope="module")
def wide():
    """140 samples, 4,200 records, no two samples alike: the model's table made once and left unchanged"""
    case = grm_cases._case("wide", grm_cases.random_dosage(4200, 140, seed=9), 140, maf_ppm=10000, min_n=2)
    words = M.words_from_dosage(case["D"], 140)
    want = _want(case)
    for x in want[:2]:
        x.setflags(write=False)
    return case, words, want


def test_a_swapped_row_and_column_would_show(wide):
    """the expected table is not symmetric under a swap inside a tile, nor are the H L and L H products equal: this data can tell"""
    case, words, want = wide
    X, _, _ = M.cell_weights(case["D"], False, 10000, 2)
    h, l = M.digits(X)
    hl = h.T @ l
    assert (hl != hl.T).sum() > 9000
    a, b = M.pair_index(140)
    full = np.zeros((140, 140), dtype=np.int64)
    full[a, b] = want[0]
    off = full[0:32, 32:64]                                                        # a block above the diagonal: pairs (i, 32 + j)
    assert (off != off.T).sum() > 900 and len(np.unique(want[0])) > 9000


@pytest.mark.parametrize("step", [0, 63, 4097])
def test_the_same_records_in_steps(ctx, wide, step):
    case, words, want = wide
    _equal(_run(ctx, case, words, cuts=range(step, 4200, step) if step else ()), want)


def test_steps_of_one_record(ctx, wide):
    case, words, _ = wide
    head = dict(case, D=case["D"][:300])
    _equal(_run(ctx, head, words[:, :, :300], cuts=range(1, 300)), _want(head))


def test_a_step_in_several_pieces(wide):
    """the cap on a step's scratch at 1 MiB: 160 padded samples take 480 bytes a record, a piece is 2,176 records"""
    case, words, want = wide
    with Context(35, 43, 1 << 20) as c:
        assert c.get_option("grm_scratch_mb") == 384
        c.set_option("grm_scratch_mb", 1)
        _equal(_run(c, case, words), want)
        _equal(_run(c, case, words, cuts=[2176, 2177]), want)


def test_read_between_steps(ctx, wide):
    case, words, want = wide
    seen = []

    def between(c1):
        got = ctx.grm_read(140)
        head = dict(case, D=case["D"][:c1])
        _equal(got, _want(head))
        seen.append(got[2])
    _equal(_run(ctx, case, words, cuts=[64, 1000], between=between), want)
    assert seen == [64, 1000, 4200]


def test_the_device_form(ctx, wide):
    case, words, want = wide
    ds = _dev(words)
    torch.cuda.synchronize()
    ctx.grm_begin(140, False, 10000, 2)
    ctx.grm_step_device(4200, 3, ds.data_ptr())
    _equal(ctx.grm_read(140), want)
    ctx.grm_end()


def test_haploid_wide(ctx):
    D = grm_cases.random_dosage(700, 200, seed=11)
    D[D == 1] = 2
    case = grm_cases._case("haploid_wide", D, 200, haploid=True, maf_ppm=20000, min_n=5)
    _equal(_run(ctx, case, M.words_from_dosage(D, 200), cuts=[333]), _want(case))


def test_the_fold_case(ctx):
    """140,000 identical records whose h h terms pass 2^31 from 133,145 on: expected is 140,000 times the one-record table.  This is the
    64-bit fold across 16 runs of 8,768 records that add with atomics (508 samples: 136 blocks, far below GRM_FILL), not a full i32 run:
    no accumulator here goes past 16,129 x 8,768 < 2^28.  A run of GRM_MAX_RUN records without atomics is in tests/test_gpu_site_word_edges.py"""
    D, records = grm_cases.fold_case()
    n = grm_cases.FOLD_SAMPLES
    S1, N1, _, e1 = M.grm_sums(D, n)
    assert e1 == 1 and int(S1[0]) == 32608 ** 2
    words = np.ascontiguousarray(np.repeat(M.words_from_dosage(D, n), records, axis=2))
    case = dict(n_samples=n, haploid=False, maf_ppm=0, min_n=1)
    _equal(_run(ctx, case, words), (S1 * records, N1 * np.uint64(records), records, records))


# ---- the ABI: arguments, state, stats ------------------------------------------------------------------------------------------------

def test_argument_and_state_errors():
    case = next(c for c in CASES if c["name"] == "samples_65")
    words = M.words_from_dosage(case["D"], 65)
    n = words.shape[2]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    k = 65 * 66 // 2
    S, N, rec = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    q = np.zeros((n, 4), dtype=np.int16)
    with Context(35, 43, 1 << 20) as c:
        L, h = c._L, c.h
        for form in (L.mg_grm_weights, L.mg_grm_weights_device):
            for bad in ((n, 2, 0, p(words), 0, 0, 1, p(q)), (n, 2, capi.GRM_MAX_SAMPLES + 1, p(words), 0, 0, 1, p(q)), (n, 1, 65, p(words), 0, 0, 1, p(q)),
                        (n, 3, 65, p(words), 0, 0, 1, p(q)), (n, 2, 65, p(words), 0, 500001, 1, p(q)), (n, 2, 65, p(words), 0, 0, 0, p(q)),
                        (n, 2, 65, None, 0, 0, 1, p(q)), (n, 2, 65, p(words), 0, 0, 1, None)):
                assert form(h, *bad) == MG_ERR_ARG, bad
            assert form(None, n, 2, 65, p(words), 0, 0, 1, p(q)) == MG_ERR_ARG
            assert form(h, 0, 2, 65, None, 0, 0, 1, None) == 0
        assert not q.any(), "an argument error writes nothing"
        for form in (L.mg_grm_step, L.mg_grm_step_device):
            assert form(h, n, 2, p(words)) == MG_ERR_STATE, "a step without begin"
        assert L.mg_grm_read(h, p(S), p(N), p(rec)) == MG_ERR_STATE
        assert L.mg_grm_end(h) == 0, "an end without begin is legal"
        for bad in ((0, 0, 0, 1), (capi.GRM_MAX_SAMPLES + 1, 0, 0, 1), (65, 0, 500001, 1), (65, 0, 0, 0)):
            assert L.mg_grm_begin(h, *bad) == MG_ERR_ARG, bad
        assert L.mg_grm_begin(None, 65, 0, 0, 1) == MG_ERR_ARG
        assert L.mg_grm_step(h, n, 2, p(words)) == MG_ERR_STATE, "a refused begin leaves no state"
        assert L.mg_grm_begin(h, 65, 0, case["maf_ppm"], case["min_n"]) == 0
        for form in (L.mg_grm_step, L.mg_grm_step_device):
            assert form(h, n, 1, p(words)) == MG_ERR_ARG and form(h, n, 3, p(words)) == MG_ERR_ARG and form(h, n, 2, None) == MG_ERR_ARG
            assert form(None, n, 2, p(words)) == MG_ERR_ARG
        for bad in ((None, p(N), p(rec)), (p(S), None, p(rec)), (p(S), p(N), None)):
            assert L.mg_grm_read(h, *bad) == MG_ERR_ARG
        assert L.mg_grm_step(h, 0, 2, None) == 0, "no records is legal"
        assert L.mg_grm_read(h, p(S), p(N), p(rec)) == 0 and not S.any() and not N.any() and not rec.any()
        assert L.mg_grm_step(h, n, 2, p(words)) == 0
        assert L.mg_grm_read(h, p(S), p(N), p(rec)) == 0
        _equal((S, N, int(rec[0]), int(rec[1])), _want(case))
        assert L.mg_grm_begin(h, 2, 0, 0, 1) == 0, "a second begin discards the first"
        assert L.mg_grm_step(h, n, 2, p(words)) == MG_ERR_ARG and L.mg_grm_read(h, p(S), p(N), p(rec)) == 0
        assert not S[:3].any() and not rec.any()
        assert L.mg_grm_end(h) == 0
        assert L.mg_grm_step(h, n, 2, p(words)) == MG_ERR_STATE, "a step behind the end"
        assert L.mg_grm_stats(h, None) == MG_ERR_ARG


def test_grm_stats_before_and_after():
    case = next(c for c in CASES if c["name"] == "samples_64")
    words = M.words_from_dosage(case["D"], 64)
    with Context(35, 43, 1 << 20) as c:
        ms = (C.c_float * 3)(5.0, 5.0, 5.0)
        assert c._L.mg_grm_stats(c.h, ms) == MG_ERR_STATE and tuple(ms) == (0.0, 0.0, 0.0)
        c.grm_begin(64)
        c.grm_step(words)
        first = c.grm_stats()
        assert first[0] > 0 and first[1] > 0 and first[2] == 0, "no read yet"
        c.grm_read(64)
        ms = c.grm_stats()
        assert ms[:2] == first[:2] and ms[2] > 0
        c.set_option("grm_scratch_mb", 1)
        c.grm_step(np.ascontiguousarray(np.repeat(words, 200, axis=2)))              # 10,000 records: two pieces of 5,440 at most
        two = c.grm_stats()
        assert two[0] > 0 and two[1] > 0
        c.grm_end()
        assert c.grm_stats() == two


# ---- the command line -------------------------------------------------------------------------------------------------------------

from test_gpu_merged import BIN, COMMON, _cli, _no_leftovers, haploid_cohort  # noqa: E402,F401 (the fixture)
from test_gpu_site_tags import _median_gq  # noqa: E402

GRM_OPTS = ["--grm-min-maf", "0.05", "--grm-min-n", "2"]


def _rows(table):
    lines = table.split("\n")
    assert lines[-1] == "" and lines[0] + "\n" == M.HEADER
    return [l.split("\t") for l in lines[1:-1]]


def _read_gcta(base, names):
    """PATH.grm.bin, PATH.grm.N.bin, PATH.grm.id -> (float32 values, float32 counts), the id file checked against the manifest"""
    k = len(names) * (len(names) + 1) // 2
    val, cnt = np.fromfile(base + ".grm.bin", dtype=np.float32), np.fromfile(base + ".grm.N.bin", dtype=np.float32)
    assert val.shape == (k,) and cnt.shape == (k,)
    assert open(base + ".grm.id").read() == "".join("%s\t%s\n" % (n, n) for n in names)
    return val, cnt


def test_cli_grm_on_the_haploid_cohort(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    names = list(inputs)
    _cli(["index"] + COMMON + [fa, vcf, fq])

    def run(d, opts, group, env=None, out=None, fmt=()):
        d.mkdir()
        r = _cli(["call"] + COMMON + opts + group + ["--cohort"] + (out or ["--merged", str(d / "m.vcf")]) + ["--grm", str(d / "grm.tsv")] + list(fmt) + [fa, vcf, man],
                 env=dict(os.environ, **(env or {})))
        assert r == ""

    tables, q = {}, None
    for tag in ("all", "masked"):
        opts = GRM_OPTS + ([] if q is None else ["--min-gq", str(q)])
        d = tmp_path / tag
        run(d, opts, [])
        _no_leftovers(d, ["m.vcf", "grm.tsv"])
        merged = open(str(d / "m.vcf")).read()
        tables[tag] = open(str(d / "grm.tsv")).read()
        assert tables[tag] == M.grm_table_text(merged, maf_ppm=50000, min_n=2, min_gq=q), tag
        if q is None:
            for i, (group, batch) in enumerate(((["--cohort-group", "1"], "3"), (["--cohort-group", "3"], "7"), ([], "3"), ([], "7"))):
                g = tmp_path / ("g%d" % i)                                              # whatever the grouping, the batches and the chunks: the same bytes
                run(g, opts, group, env={"MALVA_GENO_BATCH": batch})
                _no_leftovers(g, ["m.vcf", "grm.tsv"])
                assert open(str(g / "grm.tsv")).read() == tables[tag], (group, batch)
                assert open(str(g / "m.vcf")).read() == merged
            q = _median_gq(merged)
    assert tables["all"] != tables["masked"], "--min-gq %d changes nothing in the table" % q
    rows = _rows(tables["all"])
    assert [(r[0], r[1]) for r in rows] == [(a, b) for i, a in enumerate(names) for b in names[i:]]
    assert any(int(r[2]) > 0 and float(r[3]) != 0 for r in rows) and any(r[3].startswith("-") for r in rows)
    merged = open(str(tmp_path / "all" / "m.vcf")).read()
    # the defaults, and -o alone, without --merged: one group, and groups of 3 + 1
    want = M.grm_table_text(merged)
    for i, group in enumerate(([], ["--cohort-group", "3"])):
        d = tmp_path / ("o%d" % i)
        run(d, [], group, out=["-o", str(d / "out")])
        _no_leftovers(d, ["out", "grm.tsv"])
        assert open(str(d / "grm.tsv")).read() == want
    # GCTA's files: float32 of the model's ratios
    _, D, haploid = M.dosage_from_vcf(merged)
    S, N, _, _ = M.grm_sums(D, len(names), haploid, 50000, 2)
    want_val, want_cnt = M.gcta_values(S, N)
    for i, group in enumerate(([], ["--cohort-group", "3"])):
        d = tmp_path / ("gcta%d" % i)
        run(d, GRM_OPTS, group, fmt=["--grm-format", "gcta"])
        _no_leftovers(d, ["m.vcf", "grm.tsv.grm.bin", "grm.tsv.grm.N.bin", "grm.tsv.grm.id"])
        val, cnt = _read_gcta(str(d / "grm.tsv"), names)
        assert np.array_equal(val.view(np.uint32), want_val.view(np.uint32)) and np.array_equal(cnt, want_cnt)
    assert (want_cnt > 0).all() and len(np.unique(want_val)) > 3
    _no_leftovers(tmp, ["haploid.fq", "dump.txt", "sim1.fq", "sim2.fq", "keep.txt", "cohort.tsv"] + [f for f in os.listdir(tmp) if f.startswith("haploid.vcf.gz")])


def test_cli_grm_on_general_blocks(tmp_path):
    """the diploid panel of tests/test_gpu_ld.py::test_cli_ld_on_general_blocks: multi-allelic records (they never enter) and heterozygous cells;
    grouped runs in batches and chunks of 7 records, and with --ld and --ibd beside it"""
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

    def run(d, group, env, more=()):
        d.mkdir()
        assert _cli(["call", "--cohort"] + group + ["--merged", str(d / "m.vcf"), "--grm", str(d / "grm.tsv"), "--grm-min-maf", "0.1"] + list(more) + common +
                    [str(data / "cohort.tsv")], env=dict(env0, **env)) == ""
    run(tmp_path / "all", [], {})
    _no_leftovers(tmp_path / "all", ["m.vcf", "grm.tsv"])
    merged = open(str(tmp_path / "all" / "m.vcf")).read()
    table = open(str(tmp_path / "all" / "grm.tsv")).read()
    assert table == M.grm_table_text(merged, maf_ppm=100000)
    rows = _rows(table)
    assert len(rows) == 6 and all(int(r[2]) > 100 for r in rows) and all(float(r[3]) > 0 for r in rows if r[0] == r[1])
    _, D, haploid = M.dosage_from_vcf(merged)
    assert not haploid and (D == 1).any() and (D < 0).all(axis=1).any(), "heterozygous cells, and records without bits"
    for i, (group, batch) in enumerate(((["--cohort-group", "2"], "7"), (["--cohort-group", "1"], "400"))):
        d = tmp_path / ("g%d" % i)
        run(d, group, {"MALVA_GENO_BATCH": batch})
        _no_leftovers(d, ["m.vcf", "grm.tsv"])
        assert open(str(d / "grm.tsv")).read() == table and open(str(d / "m.vcf")).read() == merged
    d = tmp_path / "beside"                                                        # the other tables of the same words beside it
    run(d, ["--cohort-group", "2"], {"MALVA_GENO_BATCH": "7"}, more=["--ld", str(tmp_path / "beside" / "ld.tsv"), "--ibd", str(tmp_path / "beside" / "ibd.tsv")])
    _no_leftovers(d, ["m.vcf", "grm.tsv", "ld.tsv", "ibd.tsv"])
    assert open(str(d / "grm.tsv")).read() == table
    assert not [f for f in os.listdir(data) if f.endswith(".part")]


def test_cli_the_three_tables_of_one_stream(haploid_cohort, tmp_path):
    """--ld, --ibd and --grm read one stream of site words per group: each table alone and all three together, in groups of two and as one
    group, in batches and chunks of 7 records -- the same bytes in every run that makes a table, the same merged file in all"""
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    _cli(["index"] + COMMON + [fa, vcf, fq])
    opts = {"ld": ["--ld-window", "5", "--ld-min-r2", "0"], "ibd": ["--ibd-min-records", "1", "--ibd-min-bp", "0"], "grm": GRM_OPTS}
    runs = [("ld", ["ld"], True), ("ibd", ["ibd"], True), ("grm", ["grm"], True), ("all", ["ld", "ibd", "grm"], True), ("one", ["ld", "ibd", "grm"], False)]
    tables, merged = {}, set()
    for tag, made, grouped in runs:
        d = tmp_path / tag
        d.mkdir()
        args = sum((["--" + t, str(d / (t + ".tsv"))] + opts[t] for t in made), [])
        assert _cli(["call"] + COMMON + (["--cohort-group", "2"] if grouped else []) + ["--cohort", "--merged", str(d / "m.vcf")] + args + [fa, vcf, man],
                    env=dict(os.environ, MALVA_GENO_BATCH="7")) == ""
        _no_leftovers(d, ["m.vcf"] + [t + ".tsv" for t in made])
        for t in made:
            tables.setdefault(t, []).append(open(str(d / (t + ".tsv"))).read())
        merged.add(open(str(d / "m.vcf")).read())
    assert len(merged) == 1 and len([l for l in merged.pop().split("\n") if l and l[0] != "#"]) > 3 * 7, "a few batches of 7 records"
    for t, texts in tables.items():
        assert len(texts) == 3 and len(set(texts)) == 1, "the %s table depends on the run" % t
        assert texts[0].count("\n") >= 2 and texts[0][0] == "#", "a %s table without a data line" % t
    assert not [f for d in [tmp] + [tmp_path / r[0] for r in runs] for f in os.listdir(d) if f.endswith(".part")]


def test_cli_grm_reports_and_timers(haploid_cohort, tmp_path):
    import subprocess
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    r = subprocess.run([BIN, "call"] + COMMON + ["--cohort", "--merged", str(tmp_path / "m.vcf"), "--grm", str(tmp_path / "grm.tsv"), fa, vcf, man], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, MALVA_GENO_TIMERS="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    _, D, haploid = M.dosage_from_vcf(open(str(tmp_path / "m.vcf")).read())
    _, _, seen, entered = M.grm_sums(D, D.shape[1], haploid, 10000, 2)
    assert "[malva-geno] grm: %d records seen, %d entered\n" % (seen, entered) in r.stderr and 0 < entered < seen
    assert "mg_grm_step, device ms per call" in r.stderr and "grm: pack, weights, expand and gram kernels (device)" in r.stderr


def test_cli_grm_usage_errors_write_nothing(haploid_cohort, tmp_path):
    import subprocess
    tmp, fa, vcf, fq, inputs = haploid_cohort
    man = str(tmp / "cohort.tsv")
    grm = str(tmp_path / "grm.tsv")
    base = ["call"] + COMMON + ["--cohort", "--merged", str(tmp_path / "m.vcf")]
    bad = [base + ["--grm-min-maf", "0.05"], base + ["--grm-min-n", "5"], base + ["--grm-format", "gcta"],          # a sub-option without --grm
           base + ["--grm", grm, "--grm-min-maf", "0.6"], base + ["--grm", grm, "--grm-min-maf", "0.5000001"], base + ["--grm", grm, "--grm-min-maf", "1e-2"],
           base + ["--grm", grm, "--grm-min-maf", "-0.1"], base + ["--grm", grm, "--grm-min-maf", "0.0100000"], base + ["--grm", grm, "--grm-min-maf", ""],
           base + ["--grm", grm, "--grm-min-n", "0"], base + ["--grm", grm, "--grm-min-n", "4294967296"], base + ["--grm", grm, "--grm-min-n", "x"],
           base + ["--grm", grm, "--grm-format", "bin"], base + ["--grm", grm, "--grm-format", "GCTA"],
           base + ["--grm", ""],
           ["call"] + COMMON + ["--grm", grm]]                                     # without --cohort
    for args in bad:
        r = subprocess.run([BIN] + args + [fa, vcf, man if "--cohort" in args else fq], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "malva : --grm" in r.stderr and r.stdout == "", args
        assert not os.listdir(tmp_path), args
    r = subprocess.run([BIN] + base + ["--grm-min-n", "5", fa, vcf, man], capture_output=True, text=True, timeout=120)
    assert "--grm-min-maf, --grm-min-n and --grm-format go with --grm" in r.stderr
    r = subprocess.run([BIN, "call"] + COMMON + ["--grm", grm, fa, vcf, fq], capture_output=True, text=True, timeout=120)
    assert "--grm goes with --cohort" in r.stderr
