"""Reads as `call`'s third argument, the parts that need no GPU: the library's entry points, the command line, and the check of
a FASTQ file that runs before any device is created."""
import os
import subprocess

import pytest

from malva_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
READS_ABI = ["mg_reads_begin", "mg_reads_add", "mg_reads_add_device", "mg_reads_finish", "mg_reads_export", "mg_reads_stats"]


def _bin():
    if not os.path.exists(BIN):
        pytest.fail("bin/malva-geno not built: run `make cli`")
    return BIN


def test_library_exports_reads_entry_points():
    L = capi.lib()
    for n in READS_ABI:
        assert hasattr(L, n), n
        assert n in capi.EXPORTED, n
    for m in ("reads_begin", "reads_add", "reads_add_device", "reads_finish", "reads_export", "reads_stats"):
        assert hasattr(capi.Context, m), m


def test_help_documents_reads():
    r = subprocess.run([_bin(), "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "READS" in r.stdout and "--min-count" in r.stdout and "--max-count" in r.stdout
    assert "FASTQ" in r.stdout and "@list" in r.stdout


def test_malformed_fastq_fails_before_any_device(tmp_path):
    fq = tmp_path / "bad.fq"
    fq.write_text("@r1\nACGTACGTACGT\n@r2\nACGTACGTACGT\n+\nIIIIIIIIIIII\n")   # the first record has no '+' line
    r = subprocess.run([_bin(), "call", "-k", "35", "-r", "43", os.path.join(ROOT, "tests", "golden", "haploid.fa"),
                        str(tmp_path / "none.vcf"), str(fq)], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0
    assert "%s:3" % fq in r.stderr, r.stderr
    assert "device" not in r.stderr, r.stderr                    # it stopped before any device was asked for


def test_reads_refused_beyond_packed_ref_k(tmp_path):
    fq = tmp_path / "r.fq"
    fq.write_text("@r1\nACGTACGTACGT\n+\nIIIIIIIIIIII\n")
    r = subprocess.run([_bin(), "call", "-k", "35", "-r", "65", os.path.join(ROOT, "tests", "golden", "haploid.fa"),
                        str(tmp_path / "none.vcf"), str(fq)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "-r <= 64" in r.stderr, r.stderr
