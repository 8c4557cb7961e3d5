"""Directed cases for the index-time reference scan (H11, main.cpp:383-401; ref_pack_kernel, ref_scan_packed_kernel and the
byte-wise ref_scan_kernel of csrc/scan_kernels.h behind mg_ref_scan, mg_ref_scan_resident and mg_reference_upload[_device]).  No GPU
and no product import here: tests/test_ref_scan_cases_cpu.py proves on any machine that every case holds what its name says;
tests/test_gpu_ref_scan_edges.py hands the same cases to the device, three ways each.

The restatement.  windows(contig, k, ref_k) follows the reference's loop literally -- erase(0, 1), append reference[p], append
reference[p - (ref_k - k) / 2] -- and returns (centre string, context string) per window.  With an odd ref_k - k the appended
base runs one ahead of a true slide, so the windows 1 .. k-1 test a string with a one-base gap that is no k-mer of the contig
("quirk windows"); a contig shorter than ref_k has one window whose strings are clipped.  The CPU file proves the restatement
against the oracle's mo_ref_scan.

Hit sets.  A case names a contig and the windows that must hit.  `bf` is filled with the restated centre strings of exactly those
windows -- the gapped strings of the quirk windows and the centres that hold N or lower-case letters among them -- so a device that
builds any window's string wrongly misses a bit, and one that reads beyond a contig sets one too many (the cases with neighbours
put the centres of the windows that straddle the two contigs into `bf` as well).

The condition, proved on the CPU for every case: the oracle's context filter holds exactly one set bit per claimed window, and
it equals the filter made by adding the restated contexts of the claimed windows.  So no two claimed contexts share a bit and no
unclaimed window hits `bf` by a collision.  Contigs come from a generator seeded by the case's name and a seed; where seed 0 does not
meet the condition the seed that find_seeds() finds is recorded in SEEDS (the CPU file repeats the search for the two setups where
it is cheap, the small filter and k = 9; every case's seed is held by the condition itself).  Where a long contig cannot claim all
its windows -- 2,000 windows in a filter of 1,000,003 bits collide for certain, 9-mers repeat, a 2^33-bit filter costs seconds per
case -- it claims the windows on both sides of every seam instead (`seam`).

A run of N longer than ref_k cannot be claimed as a whole: the windows inside it share one centre and one context.  That case claims
every window whose centre is not all N (their strings differ by where the run's edge lies) and leaves the all-N centre out of `bf`;
a second run, of mixed IUPAC letters, claims every window.

Not reachable at test size, not pinned: the 256 Mi-window slices of mg_ref_scan, and the second trip of the packed kernel's
grid-stride loop (more than 2^16 * 2,048 windows)."""
import zlib
from collections import namedtuple

import numpy as np

from oracle import capi as ocapi

REF_SCAN_W, TPB, MAX_PACKED_K = 8, 256, 64
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_IUPAC = np.frombuffer(b"NRYKMSWBDHV", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s[::-1].translate(_COMP)


def windows(contig, k, ref_k):
    """[(centre, context)] as main.cpp:385-400 makes them; ValueError where std::string(reference, off, k) throws"""
    off = (ref_k - k) // 2
    if off > len(contig):
        raise ValueError("contig shorter than (ref_k - k) / 2")
    centre, context = contig[off:off + k], contig[:ref_k]
    out = [(centre, context)]
    for p in range(ref_k, len(contig)):
        context = context[1:] + contig[p:p + 1]
        centre = centre[1:] + contig[p - off:p - off + 1]
        out.append((centre, context))
    return out


# ---- setups ------------------------------------------------------------------------------------------------------------------
BITS = (1 << 27) + 5
Setup = namedtuple("Setup", "name k ref_k bits table")
_SETUPS = [Setup("35-43", 35, 43, BITS, "full"), Setup("35-44", 35, 44, BITS, "full"), Setup("63-64", 63, 64, BITS, "full"), Setup("33-64", 33, 64, BITS, "full"),
           Setup("35-63", 35, 63, 1 << 27, "reduced"),                      # a power of two
           Setup("64-64", 64, 64, BITS, "reduced"), Setup("32-33", 32, 33, BITS, "reduced"), Setup("17-18", 17, 18, BITS, "reduced"), Setup("16-17", 16, 17, BITS, "reduced"),
           Setup("9-9", 9, 9, BITS, "reduced"),
           Setup("31-42", 31, 42, 1000003, "small"),                        # a small prime-sized filter: the long contigs claim their seam windows only
           Setup("21-29", 21, 29, (1 << 33) + 12345, "giant"),              # the generic modulus, 1 GiB per filter: a handful of cases
           Setup("64-65", 64, 65, BITS, "reduced"), Setup("100-128", 100, 128, BITS, "reduced")]
SETUPS = {s.name: s for s in _SETUPS}


def setup(name):
    return SETUPS[name]


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case(namedtuple("Case", "name setup seam buffer offset length hits extra err claims seams")):
    """buffer: what mg_reference_upload gets; the contig is buffer[offset : offset + length] and the host form gets it alone.
    hits: the numbers of the claimed windows; extra: further strings `bf` holds (they must hit nothing); err: the scan answers
    MG_ERR_ARG and inserts nothing"""
    __slots__ = ()

    @property
    def contig(self):
        return self.buffer[self.offset:self.offset + self.length]


def rand(n, name, seed, salt=0):
    return bytes(_ACGT[np.random.default_rng([zlib.crc32(name.encode()), seed, salt]).integers(0, 4, size=n)])


def put(contig, pos, what):
    return contig[:pos] + what + contig[pos + len(what):]


def n_windows(length, ref_k):
    return max(1, length - ref_k + 1)


# {case name: seed} of the cases whose contig of seed 0 does not meet the condition: what find_seeds() finds
SEEDS = {"100-128/len-r+2047": 2, "100-128/len-r+2048": 1, "63-64/len-r+2047-even": 1, "64-64/len-r+2046": 1, "64-64/pal-context": 1, "9-9/len-r+256": 3}


def build(seeds):
    cases = {}

    def add(S, tag, seam, length, hits="all", P=5, tail=9, seams=(), edit=None, err=False, **claims):
        """a random contig of `length` bases behind P other bases and before `tail` more; edit(contig) -> contig puts the case's
        letters in; hits: all | even | none | seam | a list of window numbers | a function of the restated windows"""
        name = "%s/%s" % (S.name, tag)
        assert name not in cases, name
        seed = seeds.get(name, 0)
        contig = rand(length, name, seed)
        if edit:
            contig = edit(contig)
            assert len(contig) == length
        nw = n_windows(length, S.ref_k)
        if err:
            want = ()
        elif callable(hits):
            want = tuple(hits(windows(contig, S.k, S.ref_k)))
        elif hits == "all":
            want = tuple(range(nw))
        elif hits == "even":
            want = tuple(range(0, nw, 2))
        elif hits == "none":
            want = ()
        elif hits == "seam":                                               # both sides of every seam a window number can lie on
            want = tuple(sorted({w for w in (0, 1, 7, 8, S.k - 1, S.k, 255, 256, 2047, 2048, nw - 2, nw - 1) if 0 <= w < nw}))
        else:
            want = tuple(hits)
            assert all(0 <= w < nw for w in want), name
        buf = rand(P, name, seed, 1) + contig + rand(tail, name, seed, 2)
        cases[name] = Case(name, S.name, seam, buf, P, length, want, (), err, claims, tuple(seams))
        return cases[name]

    for S in _SETUPS:
        k, r = S.k, S.ref_k
        d = r - k
        off, off_slide, odd = d // 2, d - d // 2, d & 1
        # (a contig of 2,000 bases repeats 9-mers: like the setups whose filter is small or costly, k = 9 claims the seam windows there)
        big = "all" if S.table in ("full", "reduced") and k >= 16 else "seam"
        giant = S.table == "giant"
        # -- length seams
        if off >= 1:
            add(S, "len-off-1", "a contig of (ref_k - k) / 2 - 1 bases: MG_ERR_ARG, nothing inserted", off - 1, err=True, seams=["err-below-off"])
        add(S, "len-off", "a contig of (ref_k - k) / 2 bases has no centre k-mer: MG_ERR_ARG, nothing inserted", off, err=True, seams=["err-at-off"])
        for n in sorted({off + 1, off + k - 1, r - 1} - {off, r}):
            if off < n < r:
                add(S, "len-short-%d" % n, "a contig of %d bases, shorter than ref_k: one window, both strings clipped" % n, n, seams=["short"], n_windows=1)
                if not giant:
                    add(S, "len-short-%d-none" % n, "the same, `bf` empty", n, hits="none", seams=["short"], n_windows=1)
        for e in (0, 1, 6, 7, 8):
            if giant and e not in (0, 7, 8):
                continue
            add(S, "len-r+%d" % e, "ref_k + %d bases: %d windows, the tail of one thread's REF_SCAN_W" % (e, e + 1), r + e, seams=["len-r", "w8-tail"], n_windows=e + 1)
        for e in (254, 255, 256):
            if giant and e != 256:
                continue
            add(S, "len-r+%d" % e, "%d windows: the byte-wise kernel's workgroup of 256" % (e + 1), r + e, seams=["wg-256"], n_windows=e + 1)
        for e in (2046, 2047, 2048):
            if giant and e != 2048:
                continue
            add(S, "len-r+%d" % e, "%d windows: the packed kernel's workgroup of 256 x 8" % (e + 1), r + e, hits=big, seams=["wg-2048"], n_windows=e + 1)
            if S.table == "full":
                add(S, "len-r+%d-even" % e, "the same, the even windows only", r + e, hits="even", seams=["wg-2048", "even"], n_windows=e + 1)
        # -- the quirk windows
        if odd:
            L = r + k + 12
            for tag, hits in (("0", [0]), ("1", [1]), ("k-1", [k - 1]), ("k", [k]), ("0-1-k-1-k", [0, 1, k - 1, k]), ("all", "all")):
                if giant and tag not in ("0-1-k-1-k", "all"):
                    continue
                # (the base the gap skips and its two neighbours differ: no gapped string equals a true k-mer at either offset)
                add(S, "quirk-" + tag, "odd ref_k - k: windows 1 .. k-1 test a gapped string, handed from the packed kernel to the byte-wise one", L, hits=hits,
                    edit=lambda c: put(c, off + k - 1, b"ACG"), seams=["quirk"], quirk=True)
        elif not giant:
            add(S, "noquirk-0-1-k", "even ref_k - k: windows 0, 1, k-1, k alone", r + k + 12, hits=[0, 1, k - 1, k], seams=["no-quirk"])
        # -- palindromes
        if k % 2 == 0:
            # contigs of period 2 are the only ones there are.  An even ref_k gives two windows with two contexts; with an odd one the
            # second context is the first one's reverse complement -- one bit -- so the contig stops after its first window
            L = r + 1 - r % 2
            for unit in (b"AT", b"CG"):
                add(S, "pal-kmers-" + unit.decode(), "every k-mer equals its reverse complement (f == frc)", L, edit=lambda c, u=unit, L=L: (u * L)[:L], seams=["pal-kmer"],
                    pal_kmers=True)
        if r % 2 == 0 and not giant:
            half = r // 2
            add(S, "pal-context", "window 30's ref_k-mer equals its reverse complement", r + 80, edit=lambda c: put(c, 30 + half, revcomp(c[30:30 + half])), seams=["pal-context"],
                pal_context=30)
        # -- one N seam on every table
        add(S, "N-r+7-P31", "an N at base ref_k + 7, the contig 31 bases into the buffer", 2 * r + 90, P=31, edit=lambda c: put(c, r + 7, b"N"), seams=["bad-base"], bad=[r + 7])
        if S.table != "full":
            continue
        # -- resident offsets
        for P in list(range(34)) + [12345]:
            add(S, "P%d" % P, "the contig %d bases into the uploaded buffer" % P, r + 70, P=P, seams=["offset-%d" % (P % 32), "o-zero" if P % 32 == 0 else "o-nonzero"])
        add(S, "ends-buffer", "the contig ends on the buffer's last byte: the span readers' last words are padding", r + 70, P=13, tail=0, seams=["buffer-end"])
        # -- neighbours
        for P in (0, 1, 31):
            nameA, nameB = "%s/nb-A%d" % (S.name, P), "%s/nb-B%d" % (S.name, P)
            lenA, lenB = 32 * ((r + 100) // 32) + P, r + k + 20
            seed = seeds.get(nameA, 0)
            A, B = rand(lenA, nameA, seed), rand(lenB, nameA, seed, 3)
            AB = A + B
            straddle = range(lenA - r + 1, lenA)                           # windows of A|B that start in A and end in B
            extra = tuple(AB[w + o:w + o + k] for w in straddle for o in sorted({off, off_slide}))
            for name, o, n in ((nameA, 0, lenA), (nameB, lenA, lenB)):
                cases[name] = Case(name, S.name, "contigs A (%d bases) and B back to back: the windows that straddle them are in `bf` and belong to neither" % lenA, AB, o, n,
                                   tuple(range(n - r + 1)), extra, False, dict(neighbour=P), ("neighbours", "B-starts-at-%d" % P) if o else ("neighbours",))
        # -- bad bases
        L = 2 * r + 90
        for pos in sorted({0, 1, r - 1, r, r + 6, r + 7, r + 8, 63, 64, 65, 70, 71, L - r - 1, L - r, L - 1}):
            for P in (0, 1, 31):
                add(S, "N%d-P%d" % (pos, P), "an N at base %d: the windows over it go to the byte-wise kernel, the others stay packed" % pos, L, P=P, edit=lambda c, q=pos: put(c, q, b"N"),
                    seams=["bad-base"] + (["bad-bit-%d" % pos] if pos in (63, 64, 70, 71) else []), bad=[pos])
        run = r + 9
        add(S, "N-run", "a run of N longer than ref_k + 8: every window whose centre is not all N", 3 * r + 60, edit=lambda c: put(c, r + 3, b"N" * run),
            hits=lambda ws: [i for i, (ce, _) in enumerate(ws) if ce != b"N" * k], seams=["bad-run"], bad=list(range(r + 3, r + 3 + run)))
        add(S, "iupac-run", "a run of mixed IUPAC letters longer than ref_k + 8", 3 * r + 60,
            edit=lambda c: put(c, r + 3, bytes(_IUPAC[np.random.default_rng(7).integers(0, len(_IUPAC), size=run)])), seams=["bad-run"], bad=list(range(r + 3, r + 3 + run)))
        add(S, "N-two", "two N exactly ref_k apart: one clean window between windows with one N each", 3 * r + 60, edit=lambda c: put(put(c, r + 5, b"N"), 2 * r + 5, b"N"),
            seams=["bad-base"], bad=[r + 5, 2 * r + 5])
        # -- lower case and IUPAC
        w = k + 5
        for letter in b"acgtnWR":
            for where, pos in (("first", w), ("last", w + r - 1), ("centre", w + off_slide + k // 2)):
                add(S, "letter-%s-%s" % (chr(letter), where), "a single %r at the %s base of window %d" % (chr(letter), where, w), r + k + 40,
                    edit=lambda c, q=pos, ch=letter: put(c, q, bytes([ch])), seams=["letters"], bad=[pos], letter=(w, where))
    return cases


SEAMS = ["err-below-off", "err-at-off", "short", "len-r", "w8-tail", "wg-256", "wg-2048", "even", "quirk", "no-quirk", "pal-kmer", "pal-context", "bad-base", "bad-bit-63",
         "bad-bit-64", "bad-bit-70", "bad-bit-71", "bad-run", "letters", "buffer-end", "neighbours", "B-starts-at-0", "B-starts-at-1", "B-starts-at-31", "o-zero", "o-nonzero"] + \
        ["offset-%d" % p for p in range(32)]


# ---- expected results --------------------------------------------------------------------------------------------------------
def bf_keys(c):
    """the strings `bf` holds: the restated centres of the claimed windows, then the case's extra strings"""
    if c.err:
        return []
    S = setup(c.setup)
    ws = windows(c.contig, S.k, S.ref_k)
    return [ws[i][0] for i in c.hits] + list(c.extra)


def oracle_bf(S, keys):
    obf = ocapi.BF(S.bits)
    for km in keys:
        obf.add_key(km)
    obf.switch_mode()
    return obf


def expected(c, octx=None):
    """(obf, octx) after the oracle's scan of the case's contig; octx given: the scan adds to it"""
    S = setup(c.setup)
    obf = oracle_bf(S, bf_keys(c))
    octx = octx or ocapi.BF(S.bits)
    if not c.err:
        ocapi.ref_scan(obf, octx, c.contig, S.k, S.ref_k)
    return obf, octx


def claimed_filter(c):
    """the context filter made from the restatement alone: the contexts of the claimed windows"""
    S = setup(c.setup)
    f = ocapi.BF(S.bits)
    if not c.err:
        ws = windows(c.contig, S.k, S.ref_k)
        for i in c.hits:
            f.add_key(ws[i][1])
    return f


def claimed_positions(c):
    """the same filter's set positions, by hashing the claimed contexts one at a time (no filter: the 2^33-bit setup costs 1 GiB each)"""
    S = setup(c.setup)
    if c.err:
        return np.zeros(0, dtype=np.uint64)
    ws = windows(c.contig, S.k, S.ref_k)
    return np.unique(np.array([ocapi.lib().mo_bf_hash(ws[i][1]) % S.bits for i in c.hits], dtype=np.uint64))


def holds(c):
    """the condition: one bit per claimed window, the oracle's filter equal to the restatement's"""
    _, octx = expected(c)
    return octx.popcount() == len(c.hits) and np.array_equal(octx.set_positions(), claimed_filter(c).set_positions())


def find_seeds(setups=None, limit=200):
    """how SEEDS was made: for every case the smallest seed whose contig meets the condition"""
    seeds, todo = {}, None
    for _ in range(limit):
        cases = build(seeds)
        bad = [c.name for c in cases.values() if (setups is None or c.setup in setups) and (todo is None or c.name in todo) and not holds(c)]
        if not bad:
            return seeds
        for name in sorted({name.replace("/nb-B", "/nb-A") for name in bad}):   # (the two neighbours share their contigs)
            seeds[name] = seeds.get(name, 0) + 1
        todo = set(bad) | {name.replace("/nb-B", "/nb-A") for name in bad} | {name.replace("/nb-A", "/nb-B") for name in bad}
    raise LookupError("no seed within the limit")


_CASES = build(SEEDS)


def case_ids(table=None):
    return [n for n, c in _CASES.items() if table is None or setup(c.setup).table in table]


def case(name):
    return _CASES[name]
