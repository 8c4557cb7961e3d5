"""`call --cohort --merged --gp` and the entries behind it, as far as a machine without a GPU sees them: the header declares and the
library exports the row encoders that take MG_CELLS_GP in their mg_cells, the binding has its GP methods, the command line lists
--gp and refuses it without --merged before any device is created.  And the tie strings tests/test_gpu_gp.py expects of the
device, from Python's own correctly rounded `%.6f`."""
import os
import re
import subprocess

from malva_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("mg_format_calls", "mg_format_calls_device", "mg_encode_calls_bcf", "mg_encode_calls_bcf_device")  # (GP: the bit MG_CELLS_GP of mg_cells.fields)


def test_library_exports_and_header_declares_the_gp_entries():
    text = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    assert re.search(r"#define\s+MG_CELLS_GP\s+1u", text) and capi.CELLS_GP == 1
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", text))
    L = capi.lib()
    for n in NAMES:
        assert n in declared, "include/malva_hip.h does not declare %s" % n
        assert hasattr(L, n), "libmalva_hip.so lacks %s" % n
        assert n in capi.EXPORTED
    for m in ("format_calls_gp", "format_calls_gp_device", "encode_calls_bcf_gp", "encode_calls_bcf_gp_device"):
        assert callable(getattr(capi.Context, m))


def test_gp_without_merged_is_refused(tmp_path):
    out = tmp_path / "o"
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "-o", str(out), "--gp", os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"),
                        str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "malva : --gp goes with --merged" in r.stderr
    assert r.stdout == "" and not os.listdir(tmp_path)
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--gp", os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"),
                        os.path.join(GOLDEN, "haploid.fq")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "malva : --gp goes with --merged" in r.stderr and r.stdout == "" and not os.listdir(tmp_path)


def test_gp_with_merged_passes_the_usage_check(tmp_path):
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "--merged", str(tmp_path / "m.vcf"), "--gp", os.path.join(GOLDEN, "haploid.fa"),
                        os.path.join(GOLDEN, "haploid.vcf.gz"), str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cohort manifest" in r.stderr and "--gp goes with" not in r.stderr
    assert not os.listdir(tmp_path)


def test_help_lists_gp():
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [l for l in r.stdout.split("\n") if l.lstrip().startswith("--gp ")]
    assert line and "--merged" in line[0], "--help does not list --gp"
    merged = r.stdout[r.stdout.index("--merged  "):r.stdout.index("--min-gq  ")]
    assert "GTS" in merged and "--gp" in merged, "the --merged paragraph does not say where the likelihoods went"


def test_the_ties_round_to_even():
    """what the GPU test expects of the exact ties: k / 128 has seven decimals, the last a 5"""
    assert "%.6f" % (1 / 128) == "0.007812" and "%.6f" % (3 / 128) == "0.023438" and "%.6f" % (127 / 128) == "0.992188"
