"""`call --cohort --merged --min-gq Q --site-tags` and the entries behind it, as far as a machine without a GPU sees them: the
library exports the masked formatter, the site counts, the INFO formatter and their timer, and the header declares them; the
command line knows both options, names them in --help and refuses them without --merged before any device is created.

The tag rules are restated here in Python (site_tags_rules below); tests/test_gpu_site_tags.py holds the device against this
restatement, so its AF rule is pinned on hand-written cases here."""
import os
import re
import subprocess

import pytest

from malva_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("mg_format_calls", "mg_format_calls_device", "mg_site_counts", "mg_site_counts_device", "mg_format_site_info",
         "mg_format_site_info_device", "mg_site_stats")


# ---- the rules, restated ----------------------------------------------------------------------------------------------------

def af_text(ac, an):
    """AC / AN rounded half up to six decimals, in integers"""
    if an == 0:
        return "."
    q = (2 * ac * 10 ** 6 + an) // (2 * an)
    if q == 0:
        return "0"
    if q == 10 ** 6:
        return "1"
    return "0." + ("%06d" % q).rstrip("0")


def info_text(ac, ns):
    """ac: the record's counts per allele, REF first; ns: its called samples"""
    an = sum(int(x) for x in ac)
    if len(ac) < 2:
        return "AN=%d;NS=%d" % (an, ns)
    return "AC=%s;AN=%d;AF=%s;NS=%d" % (",".join(str(int(x)) for x in ac[1:]), an, ",".join(af_text(int(x), an) for x in ac[1:]), ns)


@pytest.mark.parametrize("ac,an,want", [(1, 3, "0.333333"), (2, 3, "0.666667"), (1, 2, "0.5"), (0, 7, "0"), (7, 7, "1"), (1, 2000001, "0"), (0, 0, "."),
                                        (1, 2000000, "0.000001"), (1999999, 2000000, "1"), (1, 8, "0.125"), (1, 16, "0.0625"), (3, 128, "0.023438"),
                                        (1, 1000, "0.001"), (999, 1000, "0.999")])
def test_af_rule_on_hand_written_cases(ac, an, want):
    assert af_text(ac, an) == want


def test_info_rule_on_hand_written_cases():
    assert info_text([3, 1, 2], 3) == "AC=1,2;AN=6;AF=0.166667,0.333333;NS=3"
    assert info_text([0, 0], 0) == "AC=0;AN=0;AF=.;NS=0"
    assert info_text([5], 5) == "AN=5;NS=5"
    assert info_text([], 2) == "AN=0;NS=2"
    assert info_text([0, 4], 2) == "AC=4;AN=4;AF=1;NS=2"


# ---- the library and the command line ---------------------------------------------------------------------------------------

def test_library_exports_and_header_declares_the_site_tag_entries():
    text = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", text))
    L = capi.lib()
    for n in NAMES:
        assert n in declared, "include/malva_hip.h does not declare %s" % n
        assert hasattr(L, n), "libmalva_hip.so lacks %s" % n
        assert n in capi.EXPORTED
    for m in ("site_counts", "format_site_info", "site_stats"):
        assert callable(getattr(capi.Context, m))


@pytest.mark.parametrize("flags", [["--min-gq", "10"], ["--site-tags"], ["--min-gq", "10", "--site-tags"]], ids=["min-gq", "site-tags", "both"])
@pytest.mark.parametrize("cohort", [False, True], ids=["call", "cohort-o"])
def test_flags_without_merged_are_refused(tmp_path, flags, cohort):
    more = ["--cohort", "-o", str(tmp_path / "out")] if cohort else []
    r = subprocess.run([BIN, "call", "-1", "-b", "1"] + more + flags + [os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"),
                                                                         os.path.join(GOLDEN, "haploid.fq")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "malva : --min-gq and --site-tags go with --merged" in r.stderr
    assert r.stdout == "" and not os.listdir(tmp_path)


def test_min_gq_takes_an_integer(tmp_path):
    for bad in ("x", "1.5", "4294967296", ""):
        r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "--merged", str(tmp_path / "m.vcf"), "--min-gq", bad, os.path.join(GOLDEN, "haploid.fa"),
                            os.path.join(GOLDEN, "haploid.vcf.gz"), str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "malva : --min-gq takes an integer" in r.stderr, bad
    assert not os.listdir(tmp_path)


def test_flags_pass_the_usage_check_with_merged(tmp_path):
    """with --merged both are accepted (a negative Q too): the run gets as far as the manifest, which is missing"""
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "--merged", str(tmp_path / "m.vcf"), "--min-gq", "-3", "--site-tags",
                        os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"), str(tmp_path / "none.tsv")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cohort manifest" in r.stderr and "go with --merged" not in r.stderr
    assert not os.listdir(tmp_path)


def test_help_names_both():
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--min-gq", "--site-tags"):
        assert [l for l in r.stdout.split("\n") if l.lstrip().startswith(flag)], "--help does not list %s" % flag
    tail = r.stdout[r.stdout.index("--site-tags"):r.stdout.index("<kmc_output_prefix>:")]
    assert all(t in tail for t in ("AC", "AN", "AF", "NS"))
