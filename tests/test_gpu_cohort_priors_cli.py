"""`call --cohort --cohort-priors` end to end, on the two cohorts of tests/test_gpu_cohort.py: the haploid example with simulated
donors (here also two donors at a few reads' depth, counted with --min-count 1, where a read or two meets the prior) and the diploid
three-sample indel panel.  MALVA_GENO_BATCH=400: several batches; MALVA_GENO_ISO_PATH=1 adds the batches of lone records.

  --prior-iters 0 is the run without --cohort-priors, byte for byte, in every output.
  Substitution: a panel whose AF holds the table's COHORT_AF, called plainly, gives the calls of the --cohort-priors run -- the
  definition's REF rule is the panel parser's, and %.9g carries a float through the text.
  The host enumerator changes nothing."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from malva_amd import synth
from test_gpu_cohort import BIN, _cli, _sample_table

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCH = {"MALVA_GENO_BATCH": "400"}


def _haploid(tmp):
    """-> (options, fasta, vcf, manifest, third argument of index, env)"""
    from oracle import kmc_standin
    from test_gpu_reads import simulate_reads, write_dump
    fa = os.path.join(GOLDEN, "haploid.fa")
    vcf = str(tmp / "haploid.vcf.gz")
    shutil.copy(os.path.join(GOLDEN, "haploid.vcf.gz"), vcf)
    fq = str(tmp / "haploid.fq")
    shutil.copy(os.path.join(GOLDEN, "haploid.fq"), fq)
    write_dump(str(tmp / "dump.txt"), kmc_standin.count_fastq(fq, 43))
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
    simulate_reads(contigs, records, 71, str(tmp / "sim1.fq"), True)
    simulate_reads(contigs, records, 72, str(tmp / "sim2.fq"), True)
    for src, dst in (("sim1.fq", "thin1.fq"), ("sim2.fq", "thin2.fq")):            # one read in six of a donor: about 2.5x
        lines = open(str(tmp / src)).read().split("\n")
        reads = [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]
        open(str(tmp / dst), "w").write("".join("\n".join(r) + "\n" for r in reads[::6]))
    inputs = {"reads": "haploid.fq", "dump": "dump", "sim1": "sim1.fq", "sim2": "sim2.fq,sim1.fq", "thin1": "thin1.fq", "thin2": "thin2.fq"}
    (tmp / "cohort.tsv").write_text("".join("%s\t%s\n" % kv for kv in inputs.items()))
    return ["-1", "-k", "35", "-r", "43", "-b", "1", "-f", "AF", "--min-count", "1"], fa, vcf, str(tmp / "cohort.tsv"), fq, dict(os.environ, **BATCH)


def _diploid(tmp):
    panel = synth.indel_panel(1_500, seed=21, n_samples=70)
    prefix = str(tmp / "p")
    synth.write_vcf_fasta(panel, prefix)
    k, ref_k = 35, 43
    for s in range(3):
        hi, lo, cnt = _sample_table(synth.flat_kmer_table(panel, 60_000, k, ref_k, seed=5, max_records=1_200), s)
        rows = synth.unpack_ascii(hi, lo, ref_k)
        with open(str(tmp / ("s%d.txt" % s)), "w") as fh:
            for r, c in zip(rows, cnt):
                fh.write("%s\t%d\n" % (bytes(r[:ref_k]).decode(), int(c)))
    (tmp / "cohort.tsv").write_text("".join("s%d\ts%d\n" % (s, s) for s in range(3)))
    return (["-k", str(k), "-r", str(ref_k), "-b", "1"], prefix + ".fa", prefix + ".vcf", str(tmp / "cohort.tsv"), str(tmp / "s0"),
            dict(os.environ, MALVA_GENO_BF_BITS=str(1 << 26), **BATCH))


@pytest.fixture(scope="module", params=["haploid", "diploid"])
def cohort(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp(request.param)
    opts, fa, vcf, manifest, third, env = (_haploid if request.param == "haploid" else _diploid)(tmp)
    index_opts = opts[:opts.index("--min-count")] if "--min-count" in opts else opts
    _cli(["index"] + index_opts + [fa, vcf, third], env=env)
    return dict(kind=request.param, tmp=tmp, opts=opts, index_opts=index_opts, fa=fa, vcf=vcf, manifest=manifest, third=third, env=env)


def _call(c, out, extra, env=None, vcf=None, merged_format=None, tables=True):
    """one cohort run with every output under `out` -> {relative path: bytes}"""
    os.makedirs(str(out))
    args = ["call"] + c["opts"] + ["--cohort", "-o", str(out / "o"), "--merged", str(out / "merged"), "--gp", "--site-tags", "-v"]
    if merged_format:
        args += ["--merged-format", merged_format]
    if tables:
        args += ["--pairs", str(out / "pairs.tsv"), "--sample-stats", str(out / "samples.tsv")]
    assert _cli(args + extra + [c["fa"], vcf or c["vcf"], c["manifest"]], env=env or c["env"]) == ""
    files = {}
    for root, _, names in os.walk(str(out)):
        for n in names:
            files[os.path.relpath(os.path.join(root, n), str(out))] = open(os.path.join(root, n), "rb").read()
    assert not [n for n in files if n.endswith(".part")]
    return files


def test_zero_iterations_is_the_run_without_cohort_priors(cohort):
    c, tmp = cohort, cohort["tmp"]
    envs = [("", c["env"])] + ([("iso", dict(c["env"], MALVA_GENO_ISO_PATH="1"))] if c["kind"] == "diploid" else [])
    for tag, env in envs:
        for fmt in (None, "bcf") if not tag else (None,):
            name = "z%s%s" % (tag, fmt or "")
            plain = _call(c, tmp / (name + "_plain"), [], env=env, merged_format=fmt)
            zero = _call(c, tmp / (name + "_zero"), ["--cohort-priors", "--prior-iters", "0", "--priors-out", str(tmp / (name + ".tsv"))], env=env, merged_format=fmt)
            assert sorted(plain) == sorted(zero) and len(plain) >= 5
            for n in plain:
                assert plain[n] == zero[n], (name, n)
            rows = open(str(tmp / (name + ".tsv"))).read().split("\n")
            assert rows[0] == "#CHROM\tPOS\tID\tREF\tALT\tPANEL_AF\tCOHORT_AF\tN_INFORMATIVE" and rows[-1] == ""
            body = [r.split("\t") for r in rows[1:-1]]
            n_records = sum(1 for l in plain["merged"].split(b"\n") if l and not l.startswith(b"#")) if not fmt else len(body)
            assert len(body) == n_records and all(len(r) == 8 and r[5] == r[6] and r[7] == "0" for r in body)


def _records(text):
    return [l.split("\t") for l in text.decode().split("\n") if l and not l.startswith("#")]


def test_substitution_and_the_host_enumerator(cohort):
    c, tmp = cohort, cohort["tmp"]
    table = tmp / "priors.tsv"
    first = _call(c, tmp / "first", ["--cohort-priors", "--prior-weight", "1", "--priors-out", str(table)], tables=False)
    plain = _call(c, tmp / "plain", [], tables=False)
    assert not os.path.exists(str(table) + ".part")
    rows = [r.split("\t") for r in open(str(table)).read().split("\n")[1:-1]]
    assert len(rows) == len(_records(first["merged"]))
    assert [r[:5] for r in rows] == [r[:5] for r in _records(first["merged"])]      # one line per output record, in output order
    # the second panel: AF <- COHORT_AF; PANEL_AF parses back to the first panel's values
    opener = gzip.open if c["vcf"].endswith(".gz") else open
    vcf2 = str(tmp / "second.vcf")
    n_moved = at_row = 0                                                            # (the table follows the panel's order; a record the run does not print has no line)
    with opener(c["vcf"], "rt") as src, open(vcf2, "w") as dst:
        for line in src:
            f = line.rstrip("\n").split("\t")
            if not line.startswith("#") and at_row < len(rows) and f[:5] == rows[at_row][:5]:
                row = rows[at_row]
                at_row += 1
                info = f[7].split(";")
                at = [i for i, kv in enumerate(info) if kv.startswith("AF=")][0]
                if row[5] != ".":
                    panel_af = np.array([float(x) for x in info[at][3:].split(",")], dtype=np.float32)
                    assert np.array_equal(np.array([float(x) for x in row[5].split(",")], dtype=np.float32), panel_af), f[:5]
                    cohort_af = np.array([float(x) for x in row[6].split(",")], dtype=np.float32)
                    assert (cohort_af > 0).all()
                    n_moved += int((cohort_af != panel_af).any())
                    info[at] = "AF=" + row[6]
                    f[7] = ";".join(info)
                line = "\t".join(f) + "\n"
            dst.write(line)
    assert at_row == len(rows)
    assert n_moved > 0                                                              # (the diploid cohort's tables cover 1,200 of the panel's records)
    _cli(["index"] + c["index_opts"] + [c["fa"], vcf2, c["third"]], env=c["env"])
    second = _call(c, tmp / "second", [], vcf=vcf2, tables=False)
    samples = sorted(n for n in first if n.startswith("o/"))
    assert len(samples) >= 3 and sorted(n for n in second if n.startswith("o/")) == samples
    differ = 0
    for n in samples:
        a, b, p = _records(first[n]), _records(second[n]), _records(plain[n])
        assert len(a) == len(b) == len(p) == len(rows)
        for x, y in zip(a, b):
            assert x[:5] == y[:5] and x[8:] == y[8:], (n, x, y)                     # FORMAT and the sample column
        differ += sum(1 for x, y in zip(a, p) if x[8:] != y[8:])
    print("%s: %d of %d records moved, %d sample columns differ from the run without --cohort-priors" % (c["kind"], n_moved, len(rows), differ))
    assert differ > 0
    # every block enumerated on the host: the same files
    host = _call(c, tmp / "host", ["--cohort-priors", "--prior-weight", "1", "--priors-out", str(tmp / "priors_host.tsv")],
                 env=dict(c["env"], MALVA_GENO_HOST_ENUM="1"), tables=False)
    assert sorted(host) == sorted(first) and all(host[n] == first[n] for n in first)
    assert open(str(tmp / "priors_host.tsv")).read() == open(str(table)).read()


def test_one_group_only(cohort):
    """a --cohort-group below the cohort is refused before any device is created; nothing is written"""
    c, tmp = cohort, cohort["tmp"]
    out = tmp / "refused"
    r = subprocess.run([BIN, "call"] + c["opts"] + ["--cohort", "--cohort-priors", "--cohort-group", "2", "-o", str(out), "--priors-out", str(tmp / "refused.tsv"),
                                                    c["fa"], c["vcf"], c["manifest"]], capture_output=True, text=True, timeout=300, env=c["env"])
    assert r.returncode != 0 and "--cohort-group 2" in r.stderr and "--cohort-priors" in r.stderr and "HIP device" not in r.stderr
    assert not os.path.exists(str(out)) and not os.path.exists(str(tmp / "refused.tsv")) and not os.path.exists(str(tmp / "refused.tsv.part"))
