"""`call --cohort --pairs PATH` and the entries behind it, as far as a machine without a GPU sees them: the library exports the
packer, the pair counter and their timer; the command line names the option in --help and refuses it without --cohort before
any device is created.

The two definitions -- the dosage bit planes of mg_pack_dosage, the 3 x 3 tables of mg_pair_counts -- and the table's text are
restated here in plain numpy / Python and pinned on hand-written cases; tests/test_gpu_pairs.py holds the device against them."""
import os
import subprocess

import numpy as np

from malva_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("mg_pack_dosage", "mg_pack_dosage_device", "mg_pair_counts", "mg_pair_counts_device", "mg_pairs_stats")
HEADER = "#A\tB\tN\tN00\tN01\tN02\tN10\tN11\tN12\tN20\tN21\tN22\tIBS0\tIBS1\tIBS2\tKING"


# ---- the definitions, restated ------------------------------------------------------------------------------------------------

def dosage_plain(g1, g2, gq, haploid, vao, min_gq):
    """-> int [P, n]: the class 0, 1, 2 of every cell that has one, else -1"""
    g1 = np.asarray(g1, dtype=np.int64)
    P, n = g1.shape
    ok = np.broadcast_to((np.diff(np.asarray(vao, dtype=np.int64)) == 2)[None, :], (P, n)).copy()
    if min_gq is not None:
        ok &= np.asarray(gq, dtype=np.int64) >= min_gq
    ok &= (g1 == 0) | (g1 == 1)
    if haploid:
        d = 2 * g1
    else:
        g2 = np.asarray(g2, dtype=np.int64)
        ok &= (g2 == 0) | (g2 == 1)
        d = g1 + g2
    return np.where(ok, d, -1)


def pack_plain(g1, g2, gq, haploid, vao, min_gq=None):
    """-> uint64 [P, 3, W], W = (n + 63) // 64: bit v & 63 of word v >> 6 of [p, d] is set when cell (p, v) has class d"""
    d = dosage_plain(g1, g2, gq, haploid, vao, min_gq)
    P, n = d.shape
    W = (n + 63) // 64
    bits = np.zeros((P, 3, W * 64), dtype=np.uint8)
    for k in range(3):
        bits[:, k, :n] = d == k
    return np.packbits(bits, axis=-1, bitorder="little").view("<u8").reshape(P, 3, W).astype(np.uint64)


def _bits(planes):
    planes = np.ascontiguousarray(planes, dtype="<u8")
    n, _, W = planes.shape
    return np.unpackbits(planes.view(np.uint8).reshape(n, 3, W * 8), axis=-1, bitorder="little")


def pair_plain(planes_a, planes_b=None):
    """-> uint64 [n_a, n_b, 3, 3]: [i, j, da, db] = popcount(A[i, da] & B[j, db]) summed over the words (None: B is A)"""
    a = _bits(planes_a).astype(np.float64)                                        # (a sum is at most the bits of a row: exact)
    b = a if planes_b is None else _bits(planes_b).astype(np.float64)
    assert a.shape[2] < 1 << 50
    return np.einsum("idw,jew->ijde", a, b, optimize=True).round().astype(np.uint64)


def pairs_text(names, counts):
    """the table of --pairs from counts [S, S, 3, 3] (the entries i < j are read)"""
    lines = [HEADER]
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            c = [[int(x) for x in row] for row in counts[i][j]]
            n = sum(map(sum, c))
            ibs2 = c[0][0] + c[1][1] + c[2][2]
            ibs0 = c[0][2] + c[2][0]
            het = sum(c[1]) + c[0][1] + c[1][1] + c[2][1]
            king = "%.4f" % (float(c[1][1] - 2 * ibs0) / float(het)) if het else "."
            lines.append("\t".join([names[i], names[j], str(n)] + [str(x) for row in c for x in row] + [str(ibs0), str(n - ibs0 - ibs2), str(ibs2), king]))
    return "\n".join(lines) + "\n"


# ---- hand-written cases -------------------------------------------------------------------------------------------------------

# 3 samples x 6 records; record 2 has three alleles, the cell (2, 3) has GQ 10, the cell (0, 5) an allele index of -1
VAO = np.array([0, 2, 4, 7, 9, 11, 13], dtype=np.uint32)
G1 = np.array([[0, 0, 1, 1, 0, -1], [0, 1, 0, 0, 1, 0], [1, 0, 0, 1, 0, 1]], dtype=np.int32)
G2 = np.array([[0, 1, 1, 1, 1, 0], [1, 1, 2, 0, 1, 0], [1, 0, 0, 1, 1, 1]], dtype=np.int32)
GQ = np.array([[50] * 6, [50] * 6, [50, 50, 50, 10, 50, 50]], dtype=np.int32)


def _table(**cells):
    t = np.zeros((3, 3), dtype=np.uint64)
    for k, v in cells.items():
        t[int(k[1]), int(k[2])] = v
    return t


def test_pack_plain_on_a_case_small_enough_to_read():
    masked = pack_plain(G1, G2, GQ, False, VAO, min_gq=20)
    assert masked.shape == (3, 3, 1) and masked.dtype == np.uint64
    assert masked[:, :, 0].tolist() == [[1, 2 + 16, 8], [8 + 32, 1, 2 + 16], [2, 16, 1 + 32]]
    plain = pack_plain(G1, G2, GQ, False, VAO)
    assert plain[:, :, 0].tolist() == [[1, 2 + 16, 8], [8 + 32, 1, 2 + 16], [2, 16, 1 + 8 + 32]]
    hap = pack_plain(G1, None, GQ, True, VAO, min_gq=20)                           # 2 * gt1: class 1 is empty
    assert hap[:, :, 0].tolist() == [[1 + 2 + 16, 0, 8], [1 + 8 + 32, 0, 2 + 16], [2 + 16, 0, 1 + 32]]
    for p in (masked, plain, hap):
        assert not (p[:, 0] & p[:, 1]).any() and not (p[:, 0] & p[:, 2]).any() and not (p[:, 1] & p[:, 2]).any()
    # 65 records: a second word, whose bits at and beyond n stay clear
    vao = np.arange(0, 2 * 66, 2, dtype=np.uint32)
    one = pack_plain(np.ones((1, 65), dtype=np.int32), np.ones((1, 65), dtype=np.int32), None, False, vao)
    assert one[0].tolist() == [[0, 0], [0, 0], [(1 << 64) - 1, 1]]


def test_pair_plain_on_the_same_case():
    planes = pack_plain(G1, G2, GQ, False, VAO, min_gq=20)
    c = pair_plain(planes)
    assert c.shape == (3, 3, 3, 3) and c.dtype == np.uint64
    assert np.array_equal(c[0, 1], _table(N01=1, N12=2, N20=1))
    assert np.array_equal(c[0, 2], _table(N02=1, N10=1, N11=1))
    assert np.array_equal(c[1, 2], _table(N12=1, N20=1, N21=1, N02=1))
    assert np.array_equal(c[0, 0], _table(N00=1, N11=2, N22=1))
    assert np.array_equal(c, c.transpose(1, 0, 3, 2))
    assert np.array_equal(pair_plain(planes[:2], planes[1:]), c[:2, 1:])


def test_pairs_text_on_a_hand_written_table():
    planes = pack_plain(G1, G2, GQ, False, VAO, min_gq=20)
    assert pairs_text(["a", "b", "c"], pair_plain(planes)) == (
        HEADER + "\n"
        "a\tb\t4\t0\t1\t0\t0\t0\t2\t1\t0\t0\t1\t3\t0\t-0.6667\n"
        "a\tc\t3\t0\t0\t1\t1\t1\t0\t0\t0\t0\t1\t1\t1\t-0.3333\n"
        "b\tc\t4\t0\t0\t1\t0\t0\t1\t1\t1\t0\t2\t2\t0\t-2.0000\n")
    c = np.zeros((3, 3, 3, 3), dtype=np.uint64)
    c[0, 1] = _table(N00=5, N22=3, N02=1)                                         # no heterozygote on either side: no denominator
    c[0, 2] = _table(N00=10, N11=10)
    c[1, 2] = _table(N11=1 << 40, N01=1, N20=3)
    assert pairs_text(["x", "y", "z"], c) == (
        HEADER + "\n"
        "x\ty\t9\t5\t0\t1\t0\t0\t0\t0\t0\t3\t1\t0\t8\t.\n"
        "x\tz\t20\t10\t0\t0\t0\t10\t0\t0\t0\t0\t0\t0\t20\t0.5000\n"
        "y\tz\t1099511627780\t0\t1\t0\t0\t1099511627776\t0\t3\t0\t0\t3\t1\t1099511627776\t0.5000\n")
    assert pairs_text(["only"], np.zeros((1, 1, 3, 3), dtype=np.uint64)) == HEADER + "\n"


# ---- the library and the command line -------------------------------------------------------------------------------------------

def test_the_library_exports_the_pair_entries():
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTED and hasattr(L, n), n
    head = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    assert "the pair table of a multi-sample call set" in head


def test_pairs_goes_with_cohort(tmp_path):
    """refused by the usage check: no device is asked for, nothing is written"""
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--pairs", str(tmp_path / "x.tsv"), os.path.join(GOLDEN, "haploid.fa"), os.path.join(GOLDEN, "haploid.vcf.gz"),
                        os.path.join(GOLDEN, "haploid.fq")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "malva : --pairs goes with --cohort" in r.stderr
    assert "HIP device" not in r.stderr and r.stdout == ""
    assert not os.listdir(tmp_path)
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "-o", str(tmp_path / "out"), "--pairs", "", os.path.join(GOLDEN, "haploid.fa"),
                        os.path.join(GOLDEN, "haploid.vcf.gz"), str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "malva : --pairs takes a path" in r.stderr
    assert not os.listdir(tmp_path)


def test_pairs_passes_the_usage_check_with_cohort(tmp_path):
    """beside -o alone it is accepted: the run gets as far as the manifest, which is missing"""
    r = subprocess.run([BIN, "call", "-1", "-b", "1", "--cohort", "-o", str(tmp_path / "out"), "--pairs", str(tmp_path / "x.tsv"), os.path.join(GOLDEN, "haploid.fa"),
                        os.path.join(GOLDEN, "haploid.vcf.gz"), str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cohort manifest" in r.stderr and "goes with --cohort" not in r.stderr
    assert not os.listdir(tmp_path)


def test_help_names_pairs():
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [l for l in r.stdout.split("\n") if l.lstrip().startswith("--pairs")]
    assert line and "--cohort" in line[0], "--help does not list --pairs"
    tail = r.stdout[r.stdout.index("--pairs"):r.stdout.index("<kmc_output_prefix>:")]
    assert all(t in tail for t in ("IBS0", "KING", "--min-gq"))
