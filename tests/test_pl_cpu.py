"""`call --cohort --merged --pl` as far as a machine without a GPU sees it.  tests/pl_model.py -- the restatement the GPU tests hold the
device against -- is pinned here: its log_post, put under the prior and through exp, is bit for bit the oracle's raw genotype value, and
the hand cases of the definition come out.  Then the plumbing: the header declares and the library exports the new entries, the binding
has them, the command line lists --pl / --pl-cap and refuses their misuse before any device is created."""
import math
import os
import re
import struct
import subprocess

import numpy as np

import pl_model
from malva_amd import capi
from oracle import capi as ocapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("mg_phred_likelihoods", "mg_phred_likelihoods_device", "mg_pl_stats", "mg_format_calls", "mg_format_calls_device", "mg_encode_calls_bcf",
         "mg_encode_calls_bcf_device")  # (PL: the bit MG_CELLS_PL of mg_cells.fields)
M = pl_model.MISSING


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_the_model_is_the_oracle_without_its_prior():
    """exp(log_prior + lp_g) is the oracle's raw value, bit for bit, 0.0 where the sum is infinite: A in 2, 3, 4, 8, haploid and
    diploid, coverages 0..200, frequencies that include 0 and 1.  A cell the oracle answers with an early-out list (no coverage at all)
    has no raw values to compare and is skipped: at most 1 % of the cells"""
    rng = np.random.default_rng(20)
    cells = skipped = values = infinite = 0
    for A in (2, 3, 4, 8):
        for haploid in (False, True):
            for i in range(330):
                e = (0.001, 0.01, 0.1)[i % 3]
                kind = i % 11
                if kind == 0:
                    cov = rng.integers(0, 3, size=A)                               # nearly nothing
                elif kind == 1:
                    cov = np.zeros(A, dtype=np.int64)
                    cov[rng.integers(0, A)] = rng.integers(1, 201)                 # one allele alone
                elif kind == 2:
                    cov = np.full(A, 200)                                          # everything at the most
                else:
                    cov = rng.integers(0, 201, size=A)
                freq = rng.random(size=A).astype(np.float32)
                if i % 5 == 0:
                    freq[rng.integers(0, A)] = 0.0
                if i % 7 == 0:
                    freq[rng.integers(0, A)] = 1.0
                cov = [int(c) for c in cov]
                cells += 1
                want = ocapi.genotype(cov, freq, e, 200, haploid)
                order = [(a, -1) for a in range(A)] if haploid else [(a, c) for a in range(A) for c in range(a, A)]   # the reference's order
                if [(g1, g2) for g1, g2, _ in want] != order:                        # an early-out list
                    assert sum(cov) == 0
                    skipped += 1
                    continue
                for (g1, g2), (_, _, raw) in zip(order, want):
                    lp = pl_model.log_prior(freq, g1, g2) + pl_model.log_post(tuple(cov), g1, g2, e)
                    got = 0.0 if math.isinf(lp) else math.exp(lp)
                    assert _bits(got) == _bits(raw), (A, haploid, cov, list(freq), e, g1, g2, got, raw)
                    values += 1
                    infinite += math.isinf(lp)
    assert cells >= 2000 and skipped <= cells // 100, (cells, skipped)
    assert values > 10000 and infinite > 0


def test_the_constant():
    assert pl_model.K == float.fromhex("0x1.15f2ced384f29p+2") and math.nextafter(pl_model.K, 0.0) == 10 / math.log(10)


def test_hand_cases():
    """e = 0.001, diploid, cov (10, 0): 0/0 is the best; 0/1 costs 10 log10(2) = 3.01 a read -> 30; 1/1 ten reads at e / (1 - e) -> 300"""
    assert pl_model.pl_cell([10, 0], 0.001, 200, False, 255) == [0, 30, 255]
    assert pl_model.pl_cell([10, 0], 0.001, 200, False, 1000) == [0, 30, 300]
    assert pl_model.pl_cell([0, 0], 0.001, 200, False, 255) == [0, 0, 0]            # no data: not missing
    assert pl_model.pl_cell([0, 0, 0], 0.001, 200, True, 255) == [0, 0, 0]
    assert pl_model.pl_cell([7], 0.001, 200, False, 255) == [0] and pl_model.pl_cell([7], 0.001, 200, True, 255) == [0]
    assert pl_model.pl_cell([201, 0], 0.001, 200, False, 255) == [M, M, M]
    assert pl_model.pl_cell([0, 5, 201], 0.001, 200, False, 255) == [M] * 6 and pl_model.pl_cell([0, 5, 201], 0.001, 200, True, 255) == [M] * 3
    assert pl_model.pl_cell([200, 0], 0.001, 200, False, 255)[0] == 0                # exactly max_cov is genotyped
    assert pl_model.pl_cell([], 0.001, 200, False, 255) == []
    assert pl_model.pl_cell([10, 0], 0.001, 200, False, 1) == [0, 1, 1]
    # VCF order of a triallelic cell: 0/0 0/1 1/1 0/2 1/2 2/2 -- reads on allele 2 alone make 2/2 the best, the genotypes without it the worst
    # (the heterozygote's error term, e / (A - 2), is A - 1 = 2 times a homozygote's e / (A - 1): ten reads, 30 less)
    assert pl_model.pl_cell([0, 0, 10], 0.001, 200, False, 1000) == [330, 300, 330, 30, 30, 0]


def test_error_rate_zero():
    """a homozygote with error reads: lp = -inf -> the cap; with none: 0 * -inf = NaN -> missing"""
    assert pl_model.pl_cell([10, 1], 0.0, 200, False, 255) == [255, 0, 255]          # 0/0 and 1/1 both have error reads
    assert pl_model.pl_cell([10, 0], 0.0, 200, False, 255) == [M, 0, 255]            # 0/0: no error read; the heterozygote is the only finite one
    assert pl_model.pl_cell([10, 0], 0.0, 200, True, 99) == [M, M]                   # allele 0: NaN; allele 1: -inf; no finite value at all -> all missing
    assert pl_model.pl_cell([10, 3], 0.0, 200, True, 99) == [M, M]                   # both -inf: no finite value either
    assert pl_model.pl_cell([0, 0], 0.0, 200, False, 255) == [M, 0, M]               # (all zeros needs an error rate inside (0, 1))
    # e = 1: logf(1 - e) = -inf under every read that is right; nothing finite is left
    assert pl_model.pl_cell([10, 3], 1.0, 200, False, 255) == [M, M, M] and pl_model.pl_cell([10, 3], 1.0, 200, True, 255) == [M, M]


def test_library_exports_and_header_declares_the_pl_entries():
    text = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    assert re.search(r"#define\s+MG_PL_MISSING\s+INT32_MIN", text)
    assert re.search(r"#define\s+MG_CELLS_PL\s+2u", text) and capi.CELLS_PL == 2
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", text))
    L = capi.lib()
    for n in NAMES:
        assert n in declared, "include/malva_hip.h does not declare %s" % n
        assert hasattr(L, n), "libmalva_hip.so lacks %s" % n
        assert n in capi.EXPORTED
    for m in ("phred_likelihoods", "phred_likelihoods_device", "pl_stats", "format_calls_pl", "format_calls_pl_device", "encode_calls_bcf_pl",
              "encode_calls_bcf_pl_device"):
        assert callable(getattr(capi.Context, m))


def _call(tmp_path, opts):
    return subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort"] + opts + [os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"),
                                                                            str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=120)


def test_pl_without_merged_is_refused(tmp_path):
    r = _call(tmp_path, ["-o", str(tmp_path / "o"), "--pl"])
    assert r.returncode != 0 and "malva : --pl goes with --merged" in r.stderr
    assert r.stdout == "" and not os.listdir(tmp_path)
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--pl", os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"),
                        os.path.join(GOLDEN, "haploid.fq")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "malva : --pl goes with --merged" in r.stderr and r.stdout == "" and not os.listdir(tmp_path)


def test_pl_cap_is_checked(tmp_path):
    for bad in ("0", "-3", "2147483648", "12x", ""):
        r = _call(tmp_path, ["--merged", str(tmp_path / "m.vcf"), "--pl", "--pl-cap", bad])
        assert r.returncode != 0 and "--pl-cap takes a whole number 1..2147483647" in r.stderr, bad
        assert r.stdout == "" and not os.listdir(tmp_path)
    r = _call(tmp_path, ["--merged", str(tmp_path / "m.vcf"), "--pl-cap", "30"])
    assert r.returncode != 0 and "malva : --pl-cap goes with --pl" in r.stderr and not os.listdir(tmp_path)


def test_pl_with_merged_passes_the_usage_check(tmp_path):
    for opts in (["--pl"], ["--pl", "--pl-cap", "2147483647"], ["--pl", "--gp", "-v", "--min-gq", "10", "--pl-cap", "1"]):
        r = _call(tmp_path, ["--merged", str(tmp_path / "m.vcf")] + opts)
        assert r.returncode != 0 and "cohort manifest" in r.stderr and "--pl" not in r.stderr
        assert not os.listdir(tmp_path)


def test_help_lists_both_options():
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    pl = [i for i, l in enumerate(lines) if l.lstrip().startswith("--pl ")]
    cap = [i for i, l in enumerate(lines) if l.lstrip().startswith("--pl-cap ")]
    gp = [i for i, l in enumerate(lines) if l.lstrip().startswith("--gp ")]
    assert len(pl) == 1 and len(cap) == 1 and gp and gp[0] < pl[0] < cap[0]
    assert "--merged" in lines[pl[0]] and "default:255" in lines[cap[0]]
    para = r.stdout[r.stdout.index("--pl  "):r.stdout.index("--pl-cap  ")]
    assert "prior" in para and "VCF order" in para and "GT:GQ[:COVS][:GP]:PL" in para
