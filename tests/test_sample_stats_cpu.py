"""`call --cohort --sample-stats PATH` and the entry behind it, as far as a machine without a GPU sees them: the library exports
the counter and its timer; the command line names the option in --help and refuses it without --cohort before any device is
created.

The definitions -- the slot table of mg_sample_counts, the allele classes the command line derives from REF and ALT, the table's
text -- are restated here in plain numpy / Python and pinned on hand-written cases; tests/test_gpu_sample_stats.py holds the device
against them."""
import os
import subprocess

import numpy as np

from malva_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("mg_sample_counts", "mg_sample_counts_device", "mg_sample_stats")
SLOTS = 32
SLOT_NAMES = ("RECORDS MASKED BAD CALLED HOM_REF HET HOM_ALT HET_ALT TS TV INS DEL OTHER GQ_SUM COV_SUM NORMAL OVERCOV SINGLE NOCOV "
              "GQ_0 GQ_10 GQ_20 GQ_30 GQ_40 GQ_50 GQ_60 GQ_70 GQ_80 GQ_90").split()
SS = {name: k for k, name in enumerate(SLOT_NAMES)}
COLUMNS = ("RECORDS CALLED MASKED BAD HOM_REF HET HOM_ALT HET_ALT TS TV INS DEL OTHER GQ_SUM COV_SUM NORMAL OVERCOV SINGLE NOCOV "
           "GQ_0 GQ_10 GQ_20 GQ_30 GQ_40 GQ_50 GQ_60 GQ_70 GQ_80 GQ_90").split()
HEADER = "#SAMPLE\t" + "\t".join(COLUMNS) + "\tCALL_RATE\tHET_HOM\tTSTV\tMEAN_GQ\tMEAN_COV"


# ---- the definitions, restated ------------------------------------------------------------------------------------------------

def sample_counts_plain(g1, g2, gq, haploid, vao, status=None, cov=None, allele_class=None, min_gq=None):
    """-> uint64 [P, 32]: the slots of mg_sample_counts (include/malva_hip.h) for every plane; GQ_SUM in two's complement"""
    g1 = np.asarray(g1, dtype=np.int64)
    P, n = g1.shape
    g2 = g1 if haploid else np.asarray(g2, dtype=np.int64)
    q = np.asarray(gq, dtype=np.int64)
    vao = np.asarray(vao, dtype=np.int64)
    A, a0 = np.diff(vao)[None, :], vao[:-1]
    masked = q < min_gq if min_gq is not None else np.zeros((P, n), dtype=bool)
    in_range = (g1 >= 0) & (g1 < A) & (g2 >= 0) & (g2 < A)
    bad = ~masked & ~in_range
    called = ~masked & in_range
    het = called & (g1 != g2)                                                     # (haploid: g2 is g1, never)
    out = np.zeros((P, SLOTS), dtype=np.uint64)

    def put(name, cells):
        out[:, SS[name]] = cells.sum(axis=1)
    put("RECORDS", np.ones((P, n), dtype=bool))
    put("MASKED", masked)
    put("BAD", bad)
    put("CALLED", called)
    put("HOM_REF", called & (g1 == 0) & (g2 == 0))
    put("HET", het)
    put("HOM_ALT", called & (g1 != 0) & (g1 == g2))
    put("HET_ALT", het & (g1 != 0) & (g2 != 0))
    if allele_class is not None:
        cls = np.asarray(allele_class, dtype=np.int64)
        for idx, sel in ((g1, called & (g1 != 0)), (g2, het & (g2 != 0))):        # the distinct nonzero indexes of a called cell
            for p in range(P):
                c = cls[(a0 + idx[p])[sel[p]]]
                for k, name in enumerate(("TS", "TV", "INS", "DEL", "OTHER"), start=1):
                    out[p, SS[name]] += np.uint64(int((c == k).sum()))
    out[:, SS["GQ_SUM"]] = np.where(called, q, 0).sum(axis=1).astype(np.int64).view(np.uint64)
    if cov is not None and n:
        out[:, SS["COV_SUM"]] = np.asarray(cov, dtype=np.uint64)[:, int(vao[0]):int(vao[-1])].sum(axis=1, dtype=np.uint64)
    if status is not None:
        st = np.asarray(status, dtype=np.int64)
        for k, name in enumerate(("NORMAL", "OVERCOV", "SINGLE", "NOCOV")):
            put(name, st == k)
    b = np.clip(q, 0, 99) // 10
    for k in range(10):
        put("GQ_%d" % (10 * k), ~bad & (b == k))
    return out


def allele_class_plain(ref, alt):
    """the class of an ALT allele from the strings as the record prints them: 1 transition, 2 transversion, 3 insertion,
    4 deletion, 5 other"""
    if alt.startswith("<") or alt == "*" or any(c not in "ACGTacgt" for c in alt):
        return 5
    if len(ref) == 1 and len(alt) == 1:
        return 1 if {ref.upper(), alt.upper()} in ({"A", "G"}, {"C", "T"}) else 2
    if len(alt) > len(ref):
        return 3
    if len(alt) < len(ref):
        return 4
    return 5


def sample_stats_text(names, counts):
    """the table of --sample-stats from counts [S, 32]"""
    lines = [HEADER]
    for name, row in zip(names, counts):
        c = {k: int(row[SS[k]]) for k in SLOT_NAMES}
        if c["GQ_SUM"] >= 1 << 63:
            c["GQ_SUM"] -= 1 << 64
        ratio = lambda a, b: "%.4f" % (float(c[a]) / float(c[b])) if c[b] else "."
        lines.append("\t".join([name] + [str(c[k]) for k in COLUMNS] + [ratio("CALLED", "RECORDS"), ratio("HET", "HOM_ALT"), ratio("TS", "TV"),
                                                                         ratio("GQ_SUM", "CALLED"), ratio("COV_SUM", "RECORDS")]))
    return "\n".join(lines) + "\n"


# ---- hand-written cases -------------------------------------------------------------------------------------------------------

# 3 samples x 6 records, one of every allele class: TS, TV, {TS, TV} (three alleles), INS, DEL, OTHER.  With --min-gq 20:
#   a   0/0:50   0/1:30   1/2:40   1/1:250   0/1:-3 (masked)   -1/0:60 (bad)
#   b   1/1:99   1/1:10 (masked)   0/2:20   0/0:19 (masked)   1/1:100   1/1:25
#   c   0/0:-7 (masked)   2/0:40 (bad: 2 == A)   2/2:45   0/0:250   0/0:5 (masked)   0/1:33
VAO = np.array([0, 2, 4, 7, 9, 11, 13], dtype=np.uint32)
CLS = np.array([0, 1, 0, 2, 0, 1, 2, 0, 3, 0, 4, 0, 5], dtype=np.uint8)
G1 = np.array([[0, 0, 1, 1, 0, -1], [1, 1, 0, 0, 1, 1], [0, 2, 2, 0, 0, 0]], dtype=np.int32)
G2 = np.array([[0, 1, 2, 1, 1, 0], [1, 1, 2, 0, 1, 1], [0, 0, 2, 0, 0, 1]], dtype=np.int32)
GQ = np.array([[50, 30, 40, 250, -3, 60], [99, 10, 20, 19, 100, 25], [-7, 40, 45, 250, 5, 33]], dtype=np.int32)
ST = np.array([[0, 0, 0, 1, 2, 3], [0, 0, 0, 0, 0, 0], [3, 3, 7, 0, 1, 2]], dtype=np.uint8)
COV = np.array([np.arange(13), [(1 << 32) - 1] * 13, [0] * 13], dtype=np.uint32)


def _row(**slots):
    r = [0] * SLOTS
    for k, v in slots.items():
        r[SS[k]] = v % (1 << 64)
    return r


def test_sample_counts_plain_on_a_case_small_enough_to_read():
    got = sample_counts_plain(G1, G2, GQ, False, VAO, ST, COV, CLS, min_gq=20)
    assert got.shape == (3, SLOTS) and got.dtype == np.uint64
    assert got.tolist() == [
        _row(RECORDS=6, MASKED=1, BAD=1, CALLED=4, HOM_REF=1, HET=2, HOM_ALT=1, HET_ALT=1, TS=1, TV=2, INS=1, GQ_SUM=370, COV_SUM=78,
             NORMAL=3, OVERCOV=1, SINGLE=1, NOCOV=1, GQ_0=1, GQ_30=1, GQ_40=1, GQ_50=1, GQ_90=1),
        _row(RECORDS=6, MASKED=2, CALLED=4, HET=1, HOM_ALT=3, TS=1, TV=1, DEL=1, OTHER=1, GQ_SUM=244, COV_SUM=13 * ((1 << 32) - 1),
             NORMAL=6, GQ_10=2, GQ_20=2, GQ_90=2),
        _row(RECORDS=6, MASKED=2, BAD=1, CALLED=3, HOM_REF=1, HET=1, HOM_ALT=1, TV=1, OTHER=1, GQ_SUM=328, COV_SUM=0,
             NORMAL=1, OVERCOV=1, SINGLE=1, NOCOV=2, GQ_0=2, GQ_30=1, GQ_40=1, GQ_90=1)]
    # without the mask: the masked cells are called (all of them have indexes the record has), the histogram is what it was
    plain = sample_counts_plain(G1, G2, GQ, False, VAO, ST, COV, CLS)
    assert plain.tolist() == [
        _row(RECORDS=6, BAD=1, CALLED=5, HOM_REF=1, HET=3, HOM_ALT=1, HET_ALT=1, TS=1, TV=2, INS=1, DEL=1, GQ_SUM=367, COV_SUM=78,
             NORMAL=3, OVERCOV=1, SINGLE=1, NOCOV=1, GQ_0=1, GQ_30=1, GQ_40=1, GQ_50=1, GQ_90=1),
        _row(RECORDS=6, CALLED=6, HOM_REF=1, HET=1, HOM_ALT=4, TS=1, TV=2, DEL=1, OTHER=1, GQ_SUM=273, COV_SUM=13 * ((1 << 32) - 1),
             NORMAL=6, GQ_10=2, GQ_20=2, GQ_90=2),
        _row(RECORDS=6, BAD=1, CALLED=5, HOM_REF=3, HET=1, HOM_ALT=1, TV=1, OTHER=1, GQ_SUM=326, COV_SUM=0,
             NORMAL=1, OVERCOV=1, SINGLE=1, NOCOV=2, GQ_0=2, GQ_30=1, GQ_40=1, GQ_90=1)]
    for t in (got, plain):
        assert np.array_equal(t[:, SS["RECORDS"]], t[:, SS["MASKED"]] + t[:, SS["BAD"]] + t[:, SS["CALLED"]])
        assert np.array_equal(t[:, SS["GQ_0"]:SS["GQ_90"] + 1].sum(axis=1), t[:, SS["RECORDS"]] - t[:, SS["BAD"]])
        assert not t[:, len(SLOT_NAMES):].any()
    # haploid: gt2 is not read; a HOM_ALT is any nonzero index, HET and HET_ALT stay empty; the optional arrays left out
    hap = sample_counts_plain(G1, None, GQ, True, VAO, min_gq=20)
    assert hap.tolist() == [
        _row(RECORDS=6, MASKED=1, BAD=1, CALLED=4, HOM_REF=2, HOM_ALT=2, GQ_SUM=370, GQ_0=1, GQ_30=1, GQ_40=1, GQ_50=1, GQ_90=1),
        _row(RECORDS=6, MASKED=2, CALLED=4, HOM_REF=1, HOM_ALT=3, GQ_SUM=244, GQ_10=2, GQ_20=2, GQ_90=2),
        _row(RECORDS=6, MASKED=2, BAD=1, CALLED=3, HOM_REF=2, HOM_ALT=1, GQ_SUM=328, GQ_0=2, GQ_30=1, GQ_40=1, GQ_90=1)]
    # a negative sum is two's complement; no records: zeros
    neg = sample_counts_plain([[0, 0]], None, [[-5, -6]], True, [0, 2, 4])
    assert neg[0].tolist() == _row(RECORDS=2, CALLED=2, HOM_REF=2, GQ_SUM=-11, GQ_0=2) and int(neg[0, SS["GQ_SUM"]]) == (1 << 64) - 11
    assert not sample_counts_plain(np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((2, 0)), False, [0]).any()


def test_allele_class_plain():
    want = {("A", "G"): 1, ("c", "t"): 1, ("A", "C"): 2, ("A", "AT"): 3, ("AT", "A"): 4, ("AT", "GC"): 5, ("A", "<DEL>"): 5, ("A", "*"): 5, ("A", "N"): 5}
    for (ref, alt), c in want.items():
        assert allele_class_plain(ref, alt) == c, (ref, alt)
    assert allele_class_plain("G", "a") == 1 and allele_class_plain("T", "C") == 1 and allele_class_plain("G", "T") == 2


def test_sample_stats_text_on_a_hand_written_table():
    c = np.zeros((4, SLOTS), dtype=np.uint64)
    c[0] = _row(RECORDS=10, CALLED=8, MASKED=1, BAD=1, HOM_REF=3, HET=2, HOM_ALT=3, HET_ALT=1, TS=4, TV=2, INS=1, DEL=1, OTHER=1, GQ_SUM=-20, COV_SUM=(1 << 40) + 5,
                NORMAL=7, OVERCOV=1, SINGLE=1, NOCOV=1, GQ_0=2, GQ_10=1, GQ_20=1, GQ_30=1, GQ_40=1, GQ_50=1, GQ_60=1, GQ_70=0, GQ_80=0, GQ_90=1)
    c[1] = _row(RECORDS=3, MASKED=3, GQ_0=3, NOCOV=3)                             # nothing called: MEAN_GQ has no denominator
    c[2] = _row(RECORDS=4, CALLED=4, HOM_REF=2, HET=2, TS=2, GQ_SUM=400, COV_SUM=6, NORMAL=4, GQ_90=4)   # no HOM_ALT, no TV
    # c[3]: no record at all: CALL_RATE and MEAN_COV have none either
    assert sample_stats_text(["a", "b", "c", "d"], c) == (
        HEADER + "\n"
        "a\t10\t8\t1\t1\t3\t2\t3\t1\t4\t2\t1\t1\t1\t-20\t1099511627781\t7\t1\t1\t1\t2\t1\t1\t1\t1\t1\t1\t0\t0\t1\t0.8000\t0.6667\t2.0000\t-2.5000\t109951162778.1000\n"
        "b\t3\t0\t3\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t3\t3\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0.0000\t.\t.\t.\t0.0000\n"
        "c\t4\t4\t0\t0\t2\t2\t0\t0\t2\t0\t0\t0\t0\t400\t6\t4\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t4\t1.0000\t.\t.\t100.0000\t1.5000\n"
        "d" + "\t0" * 29 + "\t.\t.\t.\t.\t.\n")
    assert HEADER.split("\t")[:5] == ["#SAMPLE", "RECORDS", "CALLED", "MASKED", "BAD"] and len(HEADER.split("\t")) == 35
    assert sample_stats_text([], c[:0]) == HEADER + "\n"


# ---- the library and the command line -------------------------------------------------------------------------------------------

def test_the_library_exports_the_sample_entries():
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTED and hasattr(L, n), n
    head = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    assert "the per-sample table of a multi-sample call set" in head and "#define MG_SAMPLE_SLOTS 32" in head
    for k, name in enumerate(SLOT_NAMES):                                          # the header's slot indexes are this file's
        name = {"NORMAL": "ST_NORMAL", "OVERCOV": "ST_OVERCOV", "SINGLE": "ST_SINGLE", "NOCOV": "ST_NOCOV"}.get(name, name)
        if name.startswith("GQ_") and name not in ("GQ_SUM", "GQ_0"):
            continue
        assert "#define MG_SS_%s %d\n" % (name, k) in head or "#define MG_SS_%s %d " % (name, k) in head, name
    assert capi.SAMPLE_SLOTS == SLOTS


def test_sample_stats_goes_with_cohort(tmp_path):
    """refused by the usage check: no device is asked for, nothing is written"""
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--sample-stats", str(tmp_path / "x.tsv"), os.path.join(GOLDEN, "haploid.fa"),
                        os.path.join(GOLDEN, "haploid.vcf.gz"), os.path.join(GOLDEN, "haploid.fq")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "malva : --sample-stats goes with --cohort" in r.stderr
    assert "HIP device" not in r.stderr and r.stdout == ""
    assert not os.listdir(tmp_path)
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "-o", str(tmp_path / "out"), "--sample-stats", "", os.path.join(GOLDEN, "haploid.fa"),
                        os.path.join(GOLDEN, "haploid.vcf.gz"), str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "malva : --sample-stats takes a path" in r.stderr
    assert "HIP device" not in r.stderr
    assert not os.listdir(tmp_path)


def test_sample_stats_passes_the_usage_check_with_cohort(tmp_path):
    """beside -o alone it is accepted: the run gets as far as the manifest, which is missing"""
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "-o", str(tmp_path / "out"), "--sample-stats", str(tmp_path / "x.tsv"),
                        os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"), str(tmp_path / "none.tsv")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cohort manifest" in r.stderr and "goes with --cohort" not in r.stderr
    assert not os.listdir(tmp_path)


def test_help_names_sample_stats():
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [l for l in r.stdout.split("\n") if l.lstrip().startswith("--sample-stats")]
    assert line and "--cohort" in line[0], "--help does not list --sample-stats"
    tail = r.stdout[r.stdout.index("--sample-stats"):r.stdout.index("<kmc_output_prefix>:")]
    assert all(t in tail for t in ("CALL_RATE", "TSTV", "--min-gq", "[this build]"))
