"""Reads as `call`'s third argument, the parts that need no GPU: the library's entry points, the command line, and the check of
a FASTQ file that runs before any device is created."""
import os
import subprocess

import numpy as np
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


def _random_records(rng, ref_k, n=300):
    """reads with N runs, IUPAC codes, lower case, reverse-complement palindromes, repeats and records shorter than ref_k"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    recs = []
    for _ in range(n):
        s = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(0, 3 * ref_k + 40))).tobytes())
        for p in rng.integers(0, max(1, len(s)), size=int(rng.integers(0, 3))):
            if len(s):
                s[int(p)] = int(rng.choice(np.frombuffer(b"NRYKMSWBDHV", dtype=np.uint8)))
        if len(s) and rng.random() < 0.3:
            a = int(rng.integers(0, len(s)))
            s[a:] = s[a:].lower()
        recs.append(bytes(s))
    for _ in range(20):                                             # palindromes: a window that is its own reverse complement
        h = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ref_k // 2 + 3).tobytes()
        recs += [h + h.translate(comp)[::-1]] * int(rng.integers(1, 4))
    recs += [recs[5]] * 7 + [recs[7].lower()] * 3
    return [recs[i] for i in rng.permutation(len(recs))]


@pytest.mark.parametrize("ref_k", [9, 17, 22, 32, 33, 43, 63, 64])
def test_count_chunks_equals_standin(tmp_path, ref_k):
    """count_chunks, the exact count the device counter is tested against, agrees with the plain stand-in (count_fastq) and
    with the FASTA reader's count, over reads with N, IUPAC codes, lower case and palindromes"""
    from oracle import kmc_standin
    rng = np.random.default_rng(ref_k)
    recs = _random_records(rng, ref_k)
    fq, fa = tmp_path / "r.fq", tmp_path / "r.fa"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(recs)))
    with open(fa, "wb") as fh:                                     # multi-line records, \r\n line ends, blank lines
        for i, s in enumerate(recs):
            fh.write(b">r%d some text\r\n" % i + b"".join(s[j:j + 50] + b"\r\n" for j in range(0, len(s), 50)) + b"\n" * (i % 2))
    assert kmc_standin.read_fasta(str(fa)) == recs
    n_windows = sum(1 for s in recs for p in range(len(s) - ref_k + 1) if all(c in b"ACGTacgt" for c in s[p:p + ref_k]))
    chunks = [b"\n".join(recs[i:i + 37]) for i in range(0, len(recs), 37)]
    for ci, cs in ((1, 2 ** 32 - 1), (2, 255), (3, 4), (1, 1)):
        hi, lo, cnt, nw = kmc_standin.count_chunks(chunks, ref_k, ci, cs)
        assert nw == n_windows
        got = list(zip((bytes(r) for r in kmc_standin.decode_m(hi, lo, ref_k)), (int(c) for c in cnt)))
        assert got == kmc_standin.count_fastq(str(fq), ref_k, ci, cs), (ci, cs)
        assert got == kmc_standin.count_fasta(str(fa), ref_k, ci, cs), (ci, cs)
    # a chunk boundary ends a run as a separator byte does
    s = b"".join(recs).upper().replace(b"\n", b"")
    for cut in (1, ref_k - 1, ref_k, len(s) // 2):
        a = kmc_standin.count_chunks([s[:cut], s[cut:]], ref_k)
        b = kmc_standin.count_chunks([s[:cut] + b"\n" + s[cut:]], ref_k)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    hi, lo, cnt, nw = kmc_standin.count_chunks([], ref_k)
    assert hi.size == lo.size == cnt.size == nw == 0
    assert kmc_standin.count_chunks([b"", b"\n", b"A" * (ref_k - 1)], ref_k)[3] == 0
