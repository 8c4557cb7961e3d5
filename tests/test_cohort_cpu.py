"""`malva-geno call --cohort`: the manifest is read and checked before any device is created, so every error below shows on a
machine without a GPU -- exit status non-zero, a message naming the manifest and the line, OUTDIR left empty (not even created)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run(tmp_path, manifest_text, extra=(), out=True, name="cohort.tsv"):
    man = tmp_path / name
    if manifest_text is not None:
        man.write_text(manifest_text)
    outdir = tmp_path / "out"
    args = [BIN, "call", "-1", "-k", "35", "-r", "43", "-b", "1", "--cohort"] + (["-o", str(outdir)] if out else []) + list(extra)
    args += [os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"), str(man)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert not outdir.exists() or not os.listdir(outdir), "something was written to OUTDIR"
    return r, str(man)


@pytest.fixture
def reads(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "haploid.fq"), tmp_path / "a.fq")
    return "a.fq"


@pytest.mark.parametrize("case,line,needle", [
    ("A\t{r}\nB\tmissing.fq\n", 2, "cannot open"),
    ("A\t{r}\n\n# comment\nA\t{r}\n", 4, "listed twice"),
    ("A\t{r}\n\t{r}\n", 2, "empty sample name"),
    ("A\t{r}\nx/y\t{r}\n", 2, "contains '/'"),
    ("A\t{r}\nB {r}\n", 2, "no tab"),
])
def test_manifest_errors_name_file_and_line(tmp_path, reads, case, line, needle):
    r, man = run(tmp_path, case.format(r=reads))
    assert r.returncode != 0
    assert "%s:%d:" % (man, line) in r.stderr and needle in r.stderr, r.stderr[-800:]
    assert r.stdout == ""


def test_unreadable_manifest_and_input_that_is_not_reads(tmp_path, reads):
    r, man = run(tmp_path, None)
    assert r.returncode != 0 and "cohort manifest" in r.stderr and man in r.stderr
    (tmp_path / "junk.fq").write_text("@r1\nACGT\n")              # a FASTQ record cut short
    r, man = run(tmp_path, "A\t%s\nB\tjunk.fq\n" % reads)
    assert r.returncode != 0 and "%s:2:" % man in r.stderr


def test_usage_errors(tmp_path, reads):
    r, _ = run(tmp_path, "A\t%s\n" % reads, out=False)
    assert r.returncode != 0 and "--cohort needs -o" in r.stderr
    r, _ = run(tmp_path, "A\t%s\n" % reads, extra=["--gpus", "2"])
    assert r.returncode != 0 and "--gpus" in r.stderr
    r, _ = run(tmp_path, "A\t%s\n" % reads, extra=["--cohort-group", "65"])
    assert r.returncode != 0 and "--cohort-group" in r.stderr


def test_a_directory_is_not_an_input(tmp_path, reads):
    """the third argument of `call` must be a regular file (or a KMC database / reads list), in a manifest as on the command line"""
    (tmp_path / "adir").mkdir()
    r, man = run(tmp_path, "A\t%s\nB\tadir\n" % reads)
    assert r.returncode != 0 and "%s:2:" % man in r.stderr and "cannot open" in r.stderr
    single = subprocess.run([BIN, "call", "-1", "-b", "1", os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"), str(tmp_path / "adir")],
                            capture_output=True, text=True, timeout=120)
    assert single.returncode != 0 and "cannot open" in single.stderr and single.stdout == ""
