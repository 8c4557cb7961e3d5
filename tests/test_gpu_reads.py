"""`call` from the sample's reads: the KMC step of the reference's pipeline (MALVA:104-110, `kmc -k<r> -ci -cs -fm`) counted on
the device (mg_reads_*) must leave exactly the counters -- and so exactly the VCF -- that the scan of KMC's table of the same
reads leaves.  KMC is stood in for by oracle/kmc_standin.count_fastq."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import vcf_synth
from gpu_util import build_index_pair, map_values_by_key
from malva_amd import BF_ALT, BF_CTX, Context, synth
from oracle import kmc_standin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")


def run_cli(args, env=None):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def read_fastq_records(path):
    lines = open(path).read().split("\n")
    return [(lines[i], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def write_dump(path, table):
    with open(path, "w") as fh:
        for km, c in table:
            fh.write("%s\t%d\n" % (km.decode(), c))


def test_haploid_example_from_reads(tmp_path, golden_dir):
    """README.md:131-140 with the reads themselves as the third argument, in every READS form"""
    fa = os.path.join(golden_dir, "haploid.fa")
    vcf = str(tmp_path / "haploid.vcf.gz")
    shutil.copy(os.path.join(golden_dir, "haploid.vcf.gz"), vcf)
    fq = str(tmp_path / "haploid.fq")
    shutil.copy(os.path.join(golden_dir, "haploid.fq"), fq)
    want = open(os.path.join(golden_dir, "haploid.malva.vcf")).read()
    common = ["-1", "-k", "35", "-r", "43", "-b", "1", "-f", "AF", fa, vcf]
    run_cli(["index"] + common + [fq])
    assert run_cli(["call"] + common + [fq]) == want
    recs = read_fastq_records(fq)
    # multi-line FASTA (60 bases per line)
    fasta = str(tmp_path / "reads.fa")
    with open(fasta, "w") as fh:
        for h, s, _ in recs:
            fh.write(">" + h[1:] + "\n" + "".join(s[i:i + 60] + "\n" for i in range(0, len(s), 60)))
    assert run_cli(["call"] + common + [fasta]) == want
    # gzip
    gz = str(tmp_path / "reads.fq.gz")
    with open(fq, "rb") as a, gzip.open(gz, "wb") as b:
        b.write(a.read())
    assert run_cli(["call"] + common + [gz]) == want
    # two files, counted together; and the same through @list
    half = len(recs) // 2
    parts = []
    for name, rs in (("a.fq", recs[:half]), ("b.fq", recs[half:])):
        parts.append(str(tmp_path / name))
        with open(parts[-1], "w") as fh:
            fh.write("".join("%s\n%s\n+\n%s\n" % r for r in rs))
    assert run_cli(["call"] + common + [",".join(parts)]) == want
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as fh:
        fh.write("\n".join(parts) + "\n")
    assert run_cli(["call"] + common + ["@" + lst]) == want
    # \r\n line ends
    crlf = str(tmp_path / "crlf.fq")
    with open(crlf, "w", newline="") as fh:
        fh.write("".join("%s\r\n%s\r\n+\r\n%s\r\n" % r for r in recs))
    assert run_cli(["call"] + common + [crlf]) == want


def test_sars_cov2_c1_from_reads(tmp_path, golden_dir):
    """BASELINE config C1 with haploid.fq as READS: 15,154 records, two non-reference calls (test_gpu_cli's C1 test)"""
    fa = os.path.join(golden_dir, "reference_sarsCov2.fasta")
    vcf = str(tmp_path / "sars_cov2.vcf.gz")
    shutil.copy(os.path.join(golden_dir, "sars_cov2.vcf.gz"), vcf)
    common = ["-1", "-k", "35", "-r", "43", "-b", "1", "-f", "AF", fa, vcf, os.path.join(golden_dir, "haploid.fq")]
    run_cli(["index"] + common)
    out = run_cli(["call"] + common)
    recs = [l.split("\t") for l in out.split("\n") if l and not l.startswith("#")]
    assert len(recs) == 15154
    nonref = [(r[1], r[3], r[4], r[9]) for r in recs if not r[9].startswith("0:")]
    assert nonref == [("17747", "C", "T", "1:94"), ("17858", "A", "G", "1:100")]


def simulate_reads(contigs, records, seed, path, haploid):
    """reads of a donor that carries a random allele of every record: 100-250 nt, ~15x, 0.5 % substitutions, some N runs,
    some lower case, some reads shorter than ref_k, and one region repeated in a few thousand reads"""
    rng = np.random.default_rng(seed)
    comp = str.maketrans("ACGTacgtN", "TGCAtgcaN")
    donors = []
    for hap in range(1 if haploid else 2):
        for name, seq in contigs.items():
            out, last = [], 0
            for (cn, pos, ref, alts) in records:
                real = [a for a in alts if not a.startswith("<")]
                if cn != name or pos < last:
                    continue
                pick = int(rng.integers(0, len(real) + 1))
                out.append(seq[last:pos])
                out.append(ref if pick == 0 else real[pick - 1])
                last = pos + len(ref)
            out.append(seq[last:])
            donors.append("".join(out))
    reads = []
    for d in donors:
        n = int(len(d) * 15 / 175 / len(donors)) + 1
        for _ in range(n):
            L = int(rng.integers(100, 251))
            p = int(rng.integers(0, max(1, len(d) - L)))
            r = list(d[p:p + L])
            for i in np.nonzero(rng.random(len(r)) < 0.005)[0]:
                r[i] = "ACGT"[int(rng.integers(0, 4))]
            if rng.random() < 0.03:
                a = int(rng.integers(0, len(r)))
                r[a:a + int(rng.integers(1, 6))] = "N" * len(r[a:a + 5])
            s = "".join(r)
            if rng.random() < 0.05:
                s = s.lower()
            if rng.random() < 0.5:
                s = s.translate(comp)[::-1]
            reads.append(s)
    for _ in range(40):
        reads.append(donors[0][:int(rng.integers(5, 40))])
    rep = donors[0][len(donors[0]) // 2:len(donors[0]) // 2 + 120]
    reads += [rep] * 3000
    order = rng.permutation(len(reads))
    with open(path, "w") as fh:
        for j, i in enumerate(order):
            s = reads[i]
            fh.write("@r%d\n%s\n+\n%s\n" % (j, s, "@" * len(s)))   # (quality lines that start with '@')


@pytest.mark.parametrize("seed,haploid,k,ref_k", [(31, False, 35, 43), (32, True, 35, 43), (33, False, 31, 45), (34, False, 35, 63)])
def test_cli_reads_match_standin_table(tmp_path, seed, haploid, k, ref_k):
    prefix = str(tmp_path / "case")
    contigs, records = vcf_synth.make_case(prefix, seed, haploid=haploid, k=k, n_clusters=60, vcf_strip_chr=True)
    fq = str(tmp_path / "reads.fq")
    simulate_reads(contigs, records, seed, fq, haploid)
    full = kmc_standin.count_fastq(fq, ref_k, ci=1, cs=1 << 40)
    args = ["-k", str(k), "-r", str(ref_k), "-b", "1", "-p"] + (["-1"] if haploid else []) + [prefix + ".fa", prefix + ".vcf"]
    run_cli(["index"] + args + [fq])
    env = dict(os.environ)
    for ci, cs in ((2, 255), (1, 255), (3, 255), (2, 1000)):
        dump = str(tmp_path / ("dump_%d_%d.txt" % (ci, cs)))
        write_dump(dump, [(km, min(c, cs)) for km, c in full if c >= ci])
        want = run_cli(["call"] + args + [dump])
        opt = ["--min-count", str(ci), "--max-count", str(cs)]
        got = run_cli(["call"] + opt + args + [fq])
        assert got == want, (ci, cs)
        assert sum(1 for l in got.split("\n") if l and not l.startswith("#")) > 20
        if (ci, cs) == (2, 255):
            share = dict(env, MALVA_GENO_SHARE_DEVICE="1", MALVA_GENO_READS_CHUNK="20000")   # (records cut across many chunks)
            for g in ("2", "3"):
                assert run_cli(["call", "--gpus", g] + args + [fq], env=share) == want, g


def random_reads(genome, panel, rng, n, lo=60, hi=300):
    """reads of the genome with the panel's ALT bases put in at half of the sites"""
    g = genome.copy()
    alts = panel.pool[panel.allele_off[panel.var_allele_off[:-1] + 1]]
    take = rng.random(panel.n) < 0.5
    g[panel.pos[take]] = alts[take]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    out = []
    for _ in range(n):
        L = int(rng.integers(lo, hi))
        p = int(rng.integers(0, len(g) - L))
        s = g[p:p + L].tobytes()
        if rng.random() < 0.5:
            s = s.translate(comp)[::-1]
        out.append(s)
    return out


@pytest.fixture(scope="module")
def abi_case(tmp_path_factory):
    k, ref_k, bits = 35, 43, 1 << 22
    panel = synth.snp_panel(3000, seed=5)
    rng = np.random.default_rng(6)
    reads = random_reads(panel.genome, panel, rng, 6000)
    sat_at = int(panel.pos[10]) - ref_k // 2
    sat = panel.genome[sat_at:sat_at + ref_k].tobytes()             # a 43-mer centred on a variant ...
    reads += [sat] * 70000                                         # ... seen in 70,000 windows
    reads = [reads[i] for i in rng.permutation(len(reads))]
    fq = str(tmp_path_factory.mktemp("abi") / "r.fq")
    with open(fq, "wb") as fh:
        for i, s in enumerate(reads):
            fh.write(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    table = kmc_standin.count_fastq(fq, ref_k)
    return panel, reads, table, (k, ref_k, bits)


def _pack(table, ref_k):
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    hi = np.zeros(len(table), dtype=np.uint64)
    lo = np.zeros(len(table), dtype=np.uint64)
    cnt = np.zeros(len(table), dtype=np.uint32)
    for i, (km, c) in enumerate(table):
        v = 0
        for ch in km:
            v = (v << 2) | code[ch]
        hi[i], lo[i], cnt[i] = v >> 64, v & ((1 << 64) - 1), c
    return hi, lo, cnt


def _counters(ctx):
    return ctx.bf_export(BF_ALT), ctx.bf_export(BF_CTX), map_values_by_key(ctx)


@pytest.mark.parametrize("opts", [{}, {"reads_passes": 3}, {"reads_passes": 17}, {"reads_budget_mb": 1},
                                  {"reads_parts_log2": 0}, {"use_record_counters": 2}, {"use_record_counters": 0, "reads_passes": 1}])
def test_abi_reads_counters_equal_table_scan(abi_case, opts):
    panel, reads, table, (k, ref_k, bits) = abi_case
    hi, lo, cnt = _pack(table, ref_k)
    ref = Context(k, ref_k, bits, device=0)
    build_index_pair(ref, panel, k, ref_k, bits)
    ctx = Context(k, ref_k, bits, device=0)
    build_index_pair(ctx, panel, k, ref_k, bits)
    for name, v in opts.items():
        ctx.set_option(name, v)
        if name == "use_record_counters":
            ref.set_option(name, v)
    ref.kmc_scan(hi, lo, cnt)
    ctx.reads_begin(2, 255)
    rng = np.random.default_rng(len(opts))
    i = 0
    while i < len(reads):                                           # chunks of whole records, cut at odd places
        j = min(len(reads), i + int(rng.integers(1, 9000)))
        ctx.reads_add(b"\n".join(reads[i:j]) + b"\n")
        i = j
    n_kept = ctx.reads_finish()
    ms, counts = ctx.reads_stats()
    assert counts[4] == n_kept and counts[3] >= opts.get("reads_passes", 1)
    a, b = _counters(ref), _counters(ctx)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert a[2] == b[2]
    ehi, elo, ecnt = ctx.reads_export()
    assert len(ehi) == n_kept
    full = {(int(h), int(l)): int(c) for h, l, c in zip(hi, lo, cnt)}
    got = {(int(h), int(l)): int(c) for h, l, c in zip(ehi, elo, ecnt)}
    assert len(got) == len(ehi)
    assert all(full.get(key) == c for key, c in got.items())        # a subset of KMC's table, with its counts
    sat_key = max(full, key=lambda key: full[key])
    assert full[sat_key] == 255 and got.get(sat_key) == 255          # the satellite: 70,000 windows, capped
    if opts:
        return _close(ref, ctx)
    # every k-mer of the table whose centre is an index key is there
    keys = set(k_.decode() for k_ in map_values_by_key(ref))
    comp = str.maketrans("ACGT", "TGCA")
    off = (ref_k - k) // 2
    for key, c in full.items():
        v = (key[0] << 64) | key[1]
        s = "".join("ACGT"[(v >> (2 * (ref_k - 1 - p))) & 3] for p in range(ref_k))
        centre = s[off:off + k]
        can = min(centre, centre.translate(comp)[::-1])
        if can in keys:
            assert key in got
    _close(ref, ctx)


def _close(ref, ctx):
    ref.close()
    ctx.close()
