"""Cohort mode: one context holds the counters of several samples side by side (planes, mg_cohort_*), and the record loop
reads every plane in one pass (mg_cover_blocks_cohort_device).  The reference has no counterpart: it runs a whole `call`
(main.cpp:421-594) per sample, so what a cohort must give is that single-sample result, once per sample.  Everything is
compared EXACTLY -- counters, coverages, flags, GT, GQ, status and the likelihood doubles -- against the single-sample entry
points of the same library and, for the counters, against the oracle."""
import numpy as np
import pytest
import torch

from gpu_util import build_index_pair, map_values_by_key
from malva_amd import BF_ALT, BF_CTX, Context, MalvaError, synth
from malva_amd.resident import ResidentCohort, ResidentPanel
from oracle import capi as ocapi

pytestmark = pytest.mark.gpu
PLANES = (1, 3, 16, 17, 64)   # a cell group inside a 64-byte line, one filling a line, ones crossing lines (the planes are padded to 1, 4, 16, 32, 64)


def _export(ctx):
    n_bf, n_map = ctx.counters_size()
    t = torch.zeros(max(n_bf + n_map, 1), dtype=torch.int32, device="cuda:0")
    ctx.counters_export_device(t.data_ptr())
    ctx.synchronize()
    return t.cpu().numpy().view(np.uint32)[:n_bf + n_map], n_bf


def _sample_table(base, s):
    """table of sample s: two thirds of the base table's rows (another third for every s), counts changed per sample"""
    hi, lo, cnt = base
    keep = (np.arange(len(hi)) + s) % 3 != 0
    c = (1 + (cnt[keep].astype(np.uint64) * np.uint64(2 * s + 1) + np.uint64(7 * s)) % np.uint64(200)).astype(np.uint32)
    return np.ascontiguousarray(hi[keep]), np.ascontiguousarray(lo[keep]), c


SCAN_FORMS = {
    "direct": [],
    "no-summary": [("use_summary", 0)],
    "tickets": [("pregate_log2", 10), ("gate_log2", 14), ("use_tickets", 1), ("ticket_min_log2", 11)],
    "sub-slices": [("gate_log2", 14), ("use_sub", 1), ("sub_min_log2", 11), ("sub_words_log2", 3)],
    "partition": [("use_pregate", 2), ("pregate_log2", 10), ("gate_log2", 14), ("use_partition", 1)],
    "hit-kernel-rehash": [("use_hit_entries", 0)],
    "many-chunks": [("scan_chunk_log2", 13)],
}


PLANE_CASES = [(f, l, b) for f in sorted(SCAN_FORMS) for l in ("soa", "compact") for b in (1 << 17, 1 << 20)] + [("direct", "soa", 1 << 33), ("direct", "compact", 1 << 33)]


@pytest.mark.parametrize("form,layout,bits", PLANE_CASES)
def test_planes_hold_one_sample_each(form, layout, bits):
    """S = 5 tables (the fifth empty) into 5 planes: plane s equals a fresh single-sample context's counters after table s and
    the oracle's; a scan into one plane leaves every other plane as it was."""
    k, ref_k, S = 35, 43, 5
    panel = synth.snp_panel(3000, 31)
    base = synth.kmer_table(panel, 150000, k, ref_k, 34)
    tables = [_sample_table(base, s) for s in range(S - 1)] + [tuple(a[:0] for a in base)]
    dev = torch.device("cuda", 0)

    def scan(c, t):
        hi, lo, cnt = t
        if layout == "soa" or len(hi) == 0:
            c.kmc_scan(hi, lo, cnt)
            return
        d_hi, d_lo = (torch.from_numpy(a.view(np.int64)).to(dev) for a in (hi, lo))
        d_cnt = torch.from_numpy(cnt.view(np.int32)).to(dev)
        d_rows = torch.zeros(c.kmc_rows_bytes(len(hi)) // 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        c.kmc_pack_rows_device(d_hi.data_ptr(), d_lo.data_ptr(), d_cnt.data_ptr(), len(hi), d_rows.data_ptr())
        c.kmc_scan_rows_device(d_rows.data_ptr(), len(hi))
        c.synchronize()

    def fresh():
        c = Context(k, ref_k, bits)
        for name, value in SCAN_FORMS[form]:
            c.set_option(name, value)
        return c, build_index_pair(c, panel, k, ref_k, bits)

    want, want_oracle = [], []
    for t in tables:                      # the single-sample answers: a fresh context and a fresh oracle index per sample
        c, (obf, octx, omap) = fresh()
        scan(c, t)
        want.append(_export(c)[0])
        if len(t[0]):
            ocapi.kmc_scan_packed(octx, obf, omap, *t, k, ref_k)
        want_oracle.append((obf.counts().copy(), dict(omap.items())))
        c.close()
    assert any(w.any() for w in want) and not want[S - 1].any()
    assert not np.array_equal(want[0], want[1])

    ctx, _ = fresh()
    with ctx:
        assert ctx.cohort_info() == (0, 0)
        ctx.cohort_begin(S)
        assert ctx.cohort_info() == (S, 0)
        for s in range(S):
            assert not _plane(ctx, s)[0].any()                     # the planes start zeroed
        for s in (2, 0, 4, 1, 3):                                   # any order
            before = [_plane(ctx, j)[0] for j in range(S)]
            ctx.cohort_select(s)
            assert ctx.cohort_info() == (S, s)
            scan(ctx, tables[s])
            if len(tables[s][0]):                                   # the form the case names is the form the scan took (as tests/test_gpu_scan.py checks it)
                taken = {"tickets": "scan_tickets", "sub-slices": "scan_subs", "partition": "scan_bins"}
                for f, opt in taken.items():
                    want_form = f == form and not (f == "partition" and layout == "compact")   # (the partition form takes SoA tables only: compact rows go direct)
                    assert (ctx.get_option(opt) > 0) == want_form, "%s: %s = %d" % (form, opt, ctx.get_option(opt))
            for j in range(S):
                got, n_bf = _plane(ctx, j)
                assert np.array_equal(got, want[j] if j == s else before[j]), "plane %d after the scan into plane %d" % (j, s)
        for s in range(S):                                          # the per-plane exports of the ASCII interface, against the oracle
            ctx.cohort_select(s)
            assert np.array_equal(ctx.bf_export(BF_ALT)[3], want_oracle[s][0])
            assert map_values_by_key(ctx) == want_oracle[s][1]
        # reset and import act on the selected plane alone
        ctx.cohort_select(1)
        ctx.counters_reset()
        assert not _plane(ctx, 1)[0].any() and np.array_equal(_plane(ctx, 0)[0], want[0]) and np.array_equal(_plane(ctx, 2)[0], want[2])
        t = torch.from_numpy(want[3].view(np.int32).copy()).to(dev)
        ctx.cohort_select(1)
        ctx.counters_import_device(t.data_ptr())
        assert np.array_equal(_plane(ctx, 1)[0], want[3]) and np.array_equal(_plane(ctx, 3)[0], want[3]) and np.array_equal(_plane(ctx, 0)[0], want[0])
        with pytest.raises(MalvaError):
            ctx.cohort_select(S)
        with pytest.raises(MalvaError):
            ctx.cohort_begin(2)                                     # already in cohort mode
        ctx.cohort_end()
        assert ctx.cohort_info() == (0, 0)
        assert not _export(ctx)[0].any()                            # the single-sample vectors are back, zeroed
        scan(ctx, tables[0])
        assert np.array_equal(_export(ctx)[0], want[0])
        with pytest.raises(MalvaError):
            ctx.cohort_begin(65)
        with pytest.raises(MalvaError):
            ctx.cohort_begin(0)


def _plane(ctx, s):
    ctx.cohort_select(s)
    return _export(ctx)


def test_planes_through_reads_counting():
    """mg_reads_* ends in the same scan: reads of sample s counted into plane s give what a single-sample context gives"""
    from test_gpu_reads import random_reads
    k, ref_k, bits, S = 35, 43, 1 << 22, 3
    panel = synth.snp_panel(3000, seed=5)
    samples = [random_reads(panel.genome, panel, np.random.default_rng(60 + s), 4000) for s in range(S)]

    def count(c, reads):
        c.reads_begin(2, 255)
        for i in range(0, len(reads), 1500):
            c.reads_add(b"\n".join(reads[i:i + 1500]) + b"\n")
        return c.reads_finish()

    want = []
    for reads in samples:
        with Context(k, ref_k, bits) as c:
            build_index_pair(c, panel, k, ref_k, bits)
            assert count(c, reads) > 1000
            want.append(_export(c)[0])
    assert want[0].any() and not np.array_equal(want[0], want[1])
    with Context(k, ref_k, bits) as ctx:
        build_index_pair(ctx, panel, k, ref_k, bits)
        ctx.cohort_begin(S)
        for s in range(S):
            ctx.cohort_select(s)
            ctx.reads_begin(2, 255)
            with pytest.raises(MalvaError):
                ctx.cohort_select((s + 1) % S)                      # not while a count is open
            ctx.reads_add(b"\n".join(samples[s]) + b"\n")
            ctx.reads_finish()
        for s in range(S):
            assert np.array_equal(_plane(ctx, s)[0], want[s])
        ctx.cohort_end()


# ---- the record loop over all planes -------------------------------------------------------------------------------------

def _recipe(name):
    """-> panel, k, ref_k, haploid, bits, rows of the base table, records planted"""
    if name == "c3-isolated":
        return synth.snp_panel(200_000, seed=3), 35, 43, False, 1 << 30, 1_500_000, 60_000
    if name == "c4-clustered":
        panel = synth.clustered_snp_panel(1_200_000, seed=41, n_contigs=1)
        assert panel.pos.max() > (1 << 25)
        return panel, 35, 43, False, 1 << 30, 3_000_000, 20_000
    if name in ("c5-diploid", "c5-haploid"):
        hap = name == "c5-haploid"
        return synth.indel_panel(60_000, seed=52 + int(hap)), 35, 63, hap, 1 << 28, 2_000_000, 15_000
    if name == "non-acgt":
        panel = synth.indel_panel(12_000, seed=84)
        rng = np.random.default_rng(9)
        gpos = panel.gpos()
        for v in rng.choice(panel.n, size=1_500, replace=False):
            panel.genome[int(gpos[v]) + int(rng.integers(-30, 31))] = ord("N")
        return panel, 35, 63, False, 1 << 26, 500_000, 5_000
    raise KeyError(name)


def _flat(panel):
    """an isolated-SNP panel (synth.snp_panel) has no contig table: give it the one sequence it lies on"""
    if hasattr(panel, "contig_base"):
        return panel
    return synth.flat_from_snp_panel(panel)


@pytest.mark.parametrize("recipe", ["c3-isolated", "c4-clustered", "c5-diploid", "c5-haploid", "non-acgt"])
def test_record_loop_over_all_planes(recipe):
    """plane s of mg_cover_blocks_cohort_device == mg_cover_blocks_device after a single-sample scan of table s (coverages and
    overflow flags), and the per-plane genotype call gives the same GT, GQ, status and likelihood doubles; G in PLANES.  Then the
    way back: after mg_cohort_end a single-sample scan + cover gives what it gave before, with the records' copies on and off,
    and mg_comm_init in cohort mode fails with a message and leaves the context usable."""
    panel, k, ref_k, haploid, bits, n_rows, plant = _recipe(recipe)
    panel = _flat(panel)
    base = synth.flat_kmer_table(panel, n_rows, k, ref_k, seed=7, max_records=plant)
    dev = torch.device("cuda", 0)
    G_max = max(PLANES)
    d_tables = []
    for s in range(G_max):
        hi, lo, cnt = _sample_table(base, s)
        d_tables.append((torch.from_numpy(hi.view(np.int64)).to(dev), torch.from_numpy(lo.view(np.int64)).to(dev), torch.from_numpy(cnt.view(np.int32)).to(dev), len(hi)))

    def scan(ctx, s):
        h, l, c, n = d_tables[s]
        ctx.kmc_scan_device(h.data_ptr(), l.data_ptr(), c.data_ptr(), n)

    with Context(k, ref_k, bits) as ctx:
        ctx.set_option("blocks_round_log2", 14)                     # several rounds of tier 2 on panels this size
        ctx.reference_upload(panel.genome)
        rp = ResidentPanel(panel, 0, haploid=haploid)
        rp.index(ctx)                                               # (records handed back at index time stay out of the index: the same for both paths)
        ctx.bf_finalize(BF_ALT)
        for b, l in zip(panel.contig_base, panel.contig_len):
            ctx.ref_scan_resident(int(b), int(l))
        ctx.bf_finalize(BF_CTX)

        n_lists = np.diff(rp.t["gt_off"].cpu().numpy().view(np.uint64).astype(np.int64))

        def listed(r):
            """the likelihood doubles as bit patterns, where there is a list: a record whose status is not MG_GT_NORMAL has none, and its
            place in the buffer keeps whatever an earlier call left there"""
            return np.where(np.repeat(r["status"] == 0, n_lists), r["probs"].view(np.uint64), np.uint64(0))

        def single(s):
            ctx.counters_reset()
            scan(ctx, s)
            rp.call_step(ctx)
            r = rp.results()
            out = {key: r[key].copy() for key in ("cov", "overflow", "g1", "g2", "gq", "status")}
            out["probs"] = listed(r)
            return out

        ctx.set_option("use_record_counters", 2)
        want = [single(s) for s in range(G_max)]
        general = ctx.blocks_stats()[3]
        if recipe != "c3-isolated":
            assert general > 1000, "the recipe drew too few general records"
        # (guards against a degenerate input, not a property of the code: a sample keeps two thirds of the base table's rows, and only a
        # planted record's centred window counts towards a signature, so a tenth of the planted records with coverage is plenty)
        assert (want[0]["cov"] > 0).sum() > plant // 10 and not np.array_equal(want[0]["cov"], want[1]["cov"])
        assert ((want[0]["g1"] > 0) | (want[0]["g2"] > 0)).sum() > plant // 100
        ctx.set_option("use_record_counters", 0)
        vectors_only = single(1)
        for key in vectors_only:
            assert np.array_equal(vectors_only[key], want[1][key]), key
        ctx.set_option("use_record_counters", 2)

        for G in PLANES:
            co = ResidentCohort(rp, ctx, G)
            for s in range(G):
                co.select(s)
                scan(ctx, s)
            co.select(G - 1)
            co.call_step()
            assert ctx.cohort_info() == (G, G - 1)                  # the selected plane is left as it was
            for s in range(G):
                got = co.results(s)
                for key in ("cov", "overflow", "g1", "g2", "gq", "status"):
                    assert np.array_equal(got[key], want[s][key]), "G = %d, plane %d: %s differs" % (G, s, key)
                assert np.array_equal(listed(got), want[s]["probs"]), "G = %d, plane %d: likelihoods differ" % (G, s)
            if G == 3:
                # the single-sample record loop on a context in cohort mode reads the selected plane
                co.select(1)
                rp.cut(ctx)
                rp.cover(ctx)
                assert np.array_equal(rp.results()["cov"], want[1]["cov"])
                # cohort x multi-GPU is out of scope: an error with a message, and the context goes on working
                with pytest.raises(MalvaError, match="cohort"):
                    ctx.comm_init(0, 1, bytes(128))
                with pytest.raises(MalvaError, match="cohort"):
                    ctx.counters_view()
                co.call_step()
                assert np.array_equal(co.results(2)["cov"], want[2]["cov"])
            co.close()
            # back in single-sample mode: the records' copies are republished by the next scan
            for rec in ((2, 0) if G == 3 else (2,)):
                ctx.set_option("use_record_counters", rec)
                again = single(G % 5)
                assert ctx.get_option("record_counters_live") == (1 if rec else 0)
                for key in again:
                    assert np.array_equal(again[key], want[G % 5][key]), "after mg_cohort_end (G = %d): %s" % (G, key)
            ctx.set_option("use_record_counters", 2)
    torch.cuda.synchronize()


def test_cohort_begin_refused_in_a_group():
    k, ref_k, bits = 35, 43, 1 << 20
    panel = synth.snp_panel(500, 3)
    a, b = Context(k, ref_k, bits), Context(k, ref_k, bits)
    try:
        for c in (a, b):
            build_index_pair(c, panel, k, ref_k, bits)
        from malva_amd.capi import comm_init_all
        comm_init_all([a, b])
        with pytest.raises(MalvaError, match="multi-GPU"):
            a.cohort_begin(2)
    finally:
        a.close()
        b.close()


# ---- the command line ------------------------------------------------------------------------------------------------------

def _cli(args, env=None):
    import subprocess
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


import os  # noqa: E402
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")


@pytest.mark.parametrize("extra", [[], ["--cohort-group", "1"], ["--cohort-group", "3"], ["-v"], ["-u"], ["-v", "--cohort-group", "3", "-s", "SAMPLES"]])
def test_cli_cohort_of_four_equals_four_single_calls(tmp_path, golden_dir, extra):
    """the haploid example's reads, the same sample as a text dump, and two simulated individuals (simulate_reads of
    tests/test_gpu_reads.py on the example's reference and panel; the second given as a comma list of two files): OUTDIR/NAME.vcf is byte for byte the stdout of `call` with that input, the first also the golden VCF"""
    import shutil
    from oracle import kmc_standin
    from test_gpu_reads import simulate_reads, write_dump
    fa = os.path.join(golden_dir, "haploid.fa")
    vcf = str(tmp_path / "haploid.vcf.gz")
    shutil.copy(os.path.join(golden_dir, "haploid.vcf.gz"), vcf)
    fq = str(tmp_path / "haploid.fq")
    shutil.copy(os.path.join(golden_dir, "haploid.fq"), fq)
    write_dump(str(tmp_path / "dump.txt"), kmc_standin.count_fastq(fq, 43))
    # two simulated individuals: donors that carry a random allele of every record of the panel, reads with errors, N runs, lower case
    import gzip
    contigs, name = {}, None
    for line in open(fa):
        if line.startswith(">"):
            name = line[1:].split()[0]
            contigs[name] = []
        else:
            contigs[name].append(line.strip().upper())
    contigs = {n: "".join(v) for n, v in contigs.items()}
    records = []
    for line in gzip.open(vcf, "rt"):
        if not line.startswith("#"):
            f = line.split("\t")
            records.append((f[0], int(f[1]) - 1, f[3], f[4].split(",")))
    simulate_reads(contigs, records, 71, str(tmp_path / "sim1.fq"), True)
    simulate_reads(contigs, records, 72, str(tmp_path / "sim2.fq"), True)
    if "SAMPLES" in extra:
        hdr = [l for l in gzip.open(vcf, "rt") if l.startswith("#CHROM")][0].rstrip("\n").split("\t")[9:]
        (tmp_path / "keep.txt").write_text("\n".join(hdr[:max(1, len(hdr) // 2)]) + "\n")
        extra = [str(tmp_path / "keep.txt") if x == "SAMPLES" else x for x in extra]
    inputs = {"reads": "haploid.fq", "dump": "dump", "sim1": "sim1.fq", "sim2": "sim2.fq,sim1.fq"}
    (tmp_path / "cohort.tsv").write_text("# name<tab>input\n\n" + "".join("%s\t%s\n" % kv for kv in inputs.items()))
    single_opts = [x for i, x in enumerate(extra) if x != "--cohort-group" and (i == 0 or extra[i - 1] != "--cohort-group")]
    common = ["-1", "-k", "35", "-r", "43", "-b", "1", "-f", "AF"]
    _cli(["index"] + common + [x for x in single_opts if x not in ("-v", "-u")] + [fa, vcf, fq])
    out = tmp_path / "out"
    assert _cli(["call"] + common + extra + ["--cohort", "-o", str(out), fa, vcf, str(tmp_path / "cohort.tsv")]) == ""
    assert sorted(os.listdir(out)) == sorted(n + ".vcf" for n in inputs)
    texts = {}
    for name, inp in inputs.items():
        arg = ",".join(str(tmp_path / x) for x in inp.split(","))
        texts[name] = _cli(["call"] + common + single_opts + [fa, vcf, arg])
        assert open(str(out / (name + ".vcf"))).read() == texts[name], name
    assert texts["reads"] == texts["dump"] and texts["sim1"] != texts["reads"] and texts["sim2"] != texts["sim1"]
    if not extra:
        assert texts["reads"] == open(os.path.join(golden_dir, "haploid.malva.vcf")).read()


def test_cli_cohort_on_general_blocks_and_the_host_enumerator(tmp_path):
    """a panel of indel / MNP clusters (tiers 2 and 3), once more with every block enumerated on the host (per plane through
    mg_cohort_select + mg_lookup_cover) and with the older fused lone-variant path: three samples, groups of two"""
    panel = synth.indel_panel(1_500, seed=21, n_samples=70)   # (more than 64 samples: every record is kept on the host, so any block can be handed back)
    prefix = str(tmp_path / "p")
    synth.write_vcf_fasta(panel, prefix)
    k, ref_k = 35, 43
    names = []
    for s in range(3):
        hi, lo, cnt = _sample_table(synth.flat_kmer_table(panel, 60_000, k, ref_k, seed=5, max_records=1_200), s)
        rows = synth.unpack_ascii(hi, lo, ref_k)
        with open(str(tmp_path / ("s%d.txt" % s)), "w") as fh:
            for r, c in zip(rows, cnt):
                fh.write("%s\t%d\n" % (bytes(r[:ref_k]).decode(), int(c)))
        names.append("s%d" % s)
    (tmp_path / "cohort.tsv").write_text("".join("%s\t%s\n" % (n, n) for n in names))
    common = ["-k", str(k), "-r", str(ref_k), "-b", "1", prefix + ".fa", prefix + ".vcf"]
    env0 = dict(os.environ, MALVA_GENO_BF_BITS=str(1 << 26), MALVA_GENO_BATCH="400")
    _cli(["index"] + common + [str(tmp_path / "s0")], env=env0)
    for var in ({}, {"MALVA_GENO_HOST_ENUM": "1"}, {"MALVA_GENO_ISO_PATH": "1"}):
        env = dict(env0, **var)
        out = tmp_path / ("out" + "".join(var))
        _cli(["call", "--cohort", "--cohort-group", "2", "-o", str(out)] + common[:-2] + [prefix + ".fa", prefix + ".vcf", str(tmp_path / "cohort.tsv")], env=env)
        for n in names:
            want = _cli(["call"] + common + [str(tmp_path / n)], env=env)
            assert open(str(out / (n + ".vcf"))).read() == want, (var, n)
            assert sum(1 for l in want.split("\n") if l and not l.startswith("#") and not l.split("\t")[9].startswith("0/0")) > 0
