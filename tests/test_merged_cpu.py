"""`call --cohort --merged` and the entry behind it, as far as a machine without a GPU sees them: the library exports
mg_format_calls / mg_format_calls_device / mg_format_stats and the header declares them; the command line knows --merged, and
refuses it without --cohort before any device is created."""
import os
import re
import subprocess

from malva_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("mg_format_calls", "mg_format_calls_device", "mg_format_stats")


def test_library_exports_and_header_declares_the_format_entries():
    text = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", text))
    L = capi.lib()
    for n in NAMES:
        assert n in declared, "include/malva_hip.h does not declare %s" % n
        assert hasattr(L, n), "libmalva_hip.so lacks %s" % n
        assert n in capi.EXPORTED
    for m in ("format_calls", "format_calls_device", "format_stats"):
        assert callable(getattr(capi.Context, m))


def test_merged_without_cohort_is_refused(tmp_path):
    out = tmp_path / "m.vcf"
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--merged", str(out), os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"),
                        os.path.join(GOLDEN, "haploid.fq")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "malva : --merged goes with --cohort" in r.stderr
    assert r.stdout == "" and not out.exists() and not os.listdir(tmp_path)


def test_cohort_takes_merged_in_place_of_out_dir(tmp_path):
    """with --merged, -o is optional: the usage check passes and the run gets as far as the manifest (which is missing)"""
    man = tmp_path / "none.tsv"
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "--merged", str(tmp_path / "m.vcf"), os.path.join(GOLDEN, "haploid.fa"),
                        os.path.join(GOLDEN, "haploid.vcf.gz"), str(man)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cohort manifest" in r.stderr and "needs -o" not in r.stderr
    assert not os.listdir(tmp_path)


def test_help_names_merged():
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [l for l in r.stdout.split("\n") if "--merged" in l and l.lstrip().startswith("--merged")]
    assert line, "--help does not list --merged"
    assert "GTS" in r.stdout[r.stdout.index("--merged"):r.stdout.index("<kmc_output_prefix>:")]
    assert "[this build]" in r.stdout[r.stdout.index("--merged  "):r.stdout.index("<kmc_output_prefix>:")]
