"""Stand-in for the `kmc` counting step of the MALVA pipeline script.

TEST INFRASTRUCTURE ONLY.  The reference shells out to the third-party KMC
binary (`kmc -m<mem> -k<ref_k> -t1 -fm`, MALVA:107), which is not part of the
reference checkout and is not installed here.  Its published counting
semantics with those flags: canonical k-mers, windows containing a non-ACGT
symbol skipped, k-mers seen fewer than 2 times dropped (-ci2 default), counts
capped at 255 (-cs255 default).  This generates the *input* k-mer stream for
the end-to-end golden test; it is not part of the path being restated.
"""
from collections import Counter

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def canonical_acgt(kmer: bytes) -> bytes:
    rc = kmer.translate(_COMP)[::-1]
    return kmer if kmer < rc else rc


def count_fastq(path: str, k: int, ci: int = 2, cs: int = 255):
    """-> sorted list of (canonical k-mer bytes, count)"""
    counts = Counter()
    with open(path, "rb") as fh:
        for i, line in enumerate(fh):
            if i % 4 != 1:
                continue
            seq = line.strip().upper()
            for p in range(len(seq) - k + 1):
                w = seq[p:p + k]
                if w.strip(b"ACGT"):
                    # contains a symbol outside ACGT
                    if any(c not in b"ACGT" for c in w):
                        continue
                counts[canonical_acgt(w)] += 1
    return sorted((km, min(c, cs)) for km, c in counts.items() if c >= ci)


def read_fasta(path: str):
    """-> list of the records' sequences (bytes) of a multi-line FASTA file: a record's lines joined, '>' headers, blank
    lines and '\\r' line ends tolerated"""
    records, cur = [], None
    with open(path, "rb") as fh:
        for line in fh:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if cur is not None:
                    records.append(b"".join(cur))
                cur = []
            elif line and cur is not None:
                cur.append(line)
    if cur is not None:
        records.append(b"".join(cur))
    return records


def count_fasta(path: str, k: int, ci: int = 2, cs: int = 255):
    """count_fastq for a FASTA file (read_fasta's records) -> sorted list of (canonical k-mer bytes, count)"""
    counts = Counter()
    for seq in read_fasta(path):
        seq = seq.upper()
        for p in range(len(seq) - k + 1):
            w = seq[p:p + k]
            if w.strip(b"ACGT") and any(c not in b"ACGT" for c in w):
                continue
            counts[canonical_acgt(w)] += 1
    return sorted((km, min(c, cs)) for km, c in counts.items() if c >= ci)


def _codes(chunks):
    """the chunks' bytes as 2-bit codes (A0 C1 G2 T3; acgt folded to ACGT) and 4 for every other byte, with a 4 between two
    chunks: -> uint8 array"""
    import numpy as np
    lut = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = lut[ch + 32] = i
    parts = []
    for c in chunks:
        parts.append(lut[np.frombuffer(bytes(c), dtype=np.uint8)])
        parts.append(np.full(1, 4, dtype=np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def _pack_windows(codes, starts, k):
    """M-form (first base most significant) of the k-mers at `starts` of `codes` (all ACGT): -> (hi, lo) uint64"""
    import numpy as np
    hi = np.zeros(starts.size, dtype=np.uint64)
    lo = np.zeros(starts.size, dtype=np.uint64)
    for i in range(k):
        c = codes[starts + i].astype(np.uint64)
        sh = 2 * (k - 1 - i)
        if sh >= 64:
            hi |= c << np.uint64(sh - 64)
        else:
            lo |= c << np.uint64(sh)
    return hi, lo


def count_chunks(chunks, ref_k: int, ci: int = 1, cs: int = 2 ** 32 - 1):
    """What mg_reads_* counts from the byte chunks it is handed: every byte outside ACGTacgt and every chunk boundary ends a
    run, lower case counts as upper case, and each run's canonical ref_k-mer windows are counted (KMC -fm).  Keeps the
    k-mers seen >= ci times with their counts capped at cs, as given (the ABI's reading of 0 as 1 is not applied here).
    -> (hi, lo, cnt, n_windows): the table in M-form (first base most significant, sorted) and the number of windows
    that lie inside ACGT."""
    import numpy as np
    assert 1 <= ref_k <= 64
    codes = _codes(chunks)
    bad = np.concatenate([[0], np.cumsum(codes == 4, dtype=np.int64)])
    n = codes.size - ref_k + 1
    starts = np.nonzero(bad[ref_k:ref_k + max(n, 0)] == bad[:max(n, 0)])[0] if n > 0 else np.zeros(0, dtype=np.int64)
    fh, fl = _pack_windows(codes, starts, ref_k)
    # reverse complement: base i of the rc is 3 - base (ref_k - 1 - i) of the window
    rh, rl = _pack_windows(3 - codes[::-1], codes.size - ref_k - starts, ref_k)
    take_rc = (rh < fh) | ((rh == fh) & (rl < fl))
    hi, lo = np.where(take_rc, rh, fh), np.where(take_rc, rl, fl)
    if hi.size:
        order = np.lexsort((lo, hi))
        hi, lo = hi[order], lo[order]
        head = np.concatenate([[True], (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])])
        at = np.nonzero(head)[0]
        cnt = np.diff(np.concatenate([at, [hi.size]]))
        hi, lo = hi[at], lo[at]
    else:
        cnt = np.zeros(0, dtype=np.int64)
    keep = cnt >= ci
    cnt = np.minimum(cnt[keep], cs).astype(np.uint32)
    return hi[keep], lo[keep], cnt, int(starts.size)


def decode_m(hi, lo, k: int):
    """M-form k-mers -> uint8 [n, k] ASCII"""
    import numpy as np
    hi = np.asarray(hi, dtype=np.uint64)
    lo = np.asarray(lo, dtype=np.uint64)
    out = np.zeros((hi.size, k), dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(k):
        sh = 2 * (k - 1 - i)
        c = (hi >> np.uint64(sh - 64)) if sh >= 64 else (lo >> np.uint64(sh))
        out[:, i] = acgt[(c & np.uint64(3)).astype(np.intp)]
    return out
