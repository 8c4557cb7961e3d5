"""Directed cases for the row driver of the three encoders behind `call --cohort --merged` -- mg_format_calls (`text`),
mg_encode_calls_bcf (`bcf`), mg_format_site_info (`info`) -- and a restatement of the driver's geometry: which bytes of the output
one workgroup stages in which LDS window, and which of them leave in 16-byte stores.  No GPU and no HIP here:
tests/test_row_cases_cpu.py proves on any machine that every case holds the seams its name claims, tests/test_gpu_row_edges.py
hands the same arrays to the device.

A seam is a place where a value meets an edge of the driver: the end of a window, the first byte of a tile, the capacity, a
descriptor step, a power of ten.  A case puts one or more values there with a FILLER in front: a row whose COVS list (text, bcf) or
AC list (info) is as long as it takes, its last bytes made up of digit counts (text, info) or of wider GT / GQ types (bcf).  A tile
of 32 rows starts a window of its own, so a case holds one placement per tile; `Build.place` computes the filler from the encoder's
own item spans and records nothing that the CPU test does not check again from the finished arrays.

The item spans (`Case.spans`) come from the encoders restated below one item at a time; the CPU test holds their concatenation
against the plain formatters of the existing test files (`Case.expected`), which are imported, not copied.

PL cannot print -2147483648 (it is MG_PL_MISSING and prints `.`), so the PL split cases use -2147483647, which is as long."""
import functools
import math
import re
import struct

import numpy as np

from test_gpu_bcf import PACK, desc, gt_code, int_type, typed_int      # the pieces the plain formatters of the existing tests are made of
from test_gpu_gp import n_gt, printable
from test_site_tags_cpu import af_text

# ---- the driver's constants, restated as numbers (a test's copy: nothing here is read from the code under test) -----------------
FMT_TPB = 256            # threads of a write workgroup                 call_text_kernels.h
FMT_ROWS = 32            # rows per write workgroup (a tile)            call_text_kernels.h
FMT_WINDOW = 16384       # bytes of the LDS window                      call_text_kernels.h
SCAN_TPB = 1024          # threads of a scan workgroup                  store_kernels.h
SCAN_PER = 8             # rounds of a scan workgroup                   store_kernels.h
SCAN_CHUNK = 8192        # lengths per scan workgroup (a part)          store_kernels.h

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
PL_MISSING = INT_MIN
F_MISSING, F_EOV = 0x7F800001, 0x7F800002
PL_MISS_T = {1: -128, 2: -32768, 3: INT_MIN}
POW10 = sorted({s * v for d in range(1, 10) for v in (10 ** d - 1, 10 ** d) for s in (1, -1)} | {INT_MIN, INT_MAX})
POW10_COV = [v & 0xFFFFFFFF for v in POW10] + [(1 << 31) - 1, 1 << 31, (1 << 32) - 1]
POW10_U32 = sorted({v for d in range(1, 10) for v in (10 ** d - 1, 10 ** d)} | {(1 << 32) - 1, 0})
POW10_AN = sorted({v for d in range(1, 11) for v in (10 ** d - 1, 10 ** d)} | {1 << 32, (1 << 33) - 2, 128 * ((1 << 32) - 1)})
INT_THRESHOLDS = tuple(10 ** d for d in range(1, 10))


# ---- the geometry of fmt_write_tile and fmt_window_flush ------------------------------------------------------------------------

class Window:
    """bytes [w0, w1) of the output staged at once, the output address of w0 being `mis` past a multiple of 16; [w0, stop) leaves:
    `whole` the output offsets of the 16-byte pieces stored at once, `ragged` the (lo, hi) ranges stored byte by byte"""

    def __init__(self, w0, w1, mis, stop, whole, ragged):
        self.w0, self.w1, self.mis, self.stop, self.whole, self.ragged = w0, w1, mis, stop, whole, ragged


class Tile:
    def __init__(self, t0, t1, b0, b1, windows):
        self.t0, self.t1, self.b0, self.b1, self.windows = t0, t1, b0, b1, windows


def geometry(row_off, addr_mod16, cap, fault=None):
    """-> the tiles of a write pass over rows at row_off into a buffer whose address is addr_mod16 (mod 16) and that holds cap bytes.
    fault: 'flush-below-lo' restates a flush that stores a whole piece whose first bytes lie in front of the window."""
    n = len(row_off) - 1
    tiles = []
    for t0 in range(0, n, FMT_ROWS):
        t1 = min(t0 + FMT_ROWS, n)
        b0, b1 = int(row_off[t0]), int(row_off[t1])
        end = min(b1, cap)
        windows = []
        w0 = b0
        while w0 < end:
            mis = (addr_mod16 + w0) & 15
            w1 = b1 if b1 - w0 < FMT_WINDOW - mis else w0 + FMT_WINDOW - mis
            stop = min(w1, end)
            lo, hi = mis, mis + stop - w0
            whole, ragged = [], []
            for p0 in range(0, hi, 16):
                if (p0 >= lo or fault == "flush-below-lo") and p0 + 16 <= hi:
                    whole.append(w0 - mis + p0)
                else:
                    q0, q1 = max(p0, lo), min(p0 + 16, hi)
                    if q0 < q1:
                        ragged.append((w0 - mis + q0, w0 - mis + q1))
            windows.append(Window(w0, w1, mis, stop, whole, ragged))
            w0 = w1
        tiles.append(Tile(t0, t1, b0, b1, windows))
    return tiles


def store_map(tiles, size):
    """-> per output byte 0 (not stored), 1 (a byte store) or 2 (part of a 16-byte store), and the window's number in its tile;
    bytes a store touches in front of offset 0 are counted in the third result"""
    kind = np.zeros(size, dtype=np.uint8)
    win = np.full(size, -1, dtype=np.int64)
    outside = 0
    for t in tiles:
        for k, w in enumerate(t.windows):
            for p in w.whole:
                outside += max(0, -p) + max(0, p + 16 - size)
                kind[max(p, 0):p + 16] = 2
                win[max(p, 0):p + 16] = k
            for lo, hi in w.ragged:
                kind[lo:hi] = 1
                win[lo:hi] = k
    return kind, win, outside


def store_map_brute(row_off, addr_mod16, cap):
    """the second statement, byte by byte and without the loop: a tile's first window ends where the output address next reaches a
    multiple of 16 that is FMT_WINDOW past the piece the tile starts in, every later window is FMT_WINDOW long; a byte leaves in a
    16-byte store when its whole aligned piece lies inside what its window stores, else by itself"""
    n = len(row_off) - 1
    total = int(row_off[n])
    size = min(total, cap)
    b = np.arange(size, dtype=np.int64)
    starts = np.array([int(row_off[t0]) for t0 in range(0, n, FMT_ROWS)], dtype=np.int64)
    ends = np.array([int(row_off[min(t0 + FMT_ROWS, n)]) for t0 in range(0, n, FMT_ROWS)], dtype=np.int64)
    if size == 0:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int64)
    # (tiles without bytes share their start with the next: the last of them that starts at or in front of b is the byte's)
    t = np.searchsorted(starts, b, side="right") - 1
    while (ends[t] <= b).any():
        t = np.where(ends[t] <= b, t + 1, t)
    b0, b1 = starts[t], ends[t]
    edge0 = (addr_mod16 + b0) // 16 * 16 + FMT_WINDOW - addr_mod16        # (as an output offset)
    k = np.where(b < edge0, 0, 1 + (b - edge0) // FMT_WINDOW)
    w0 = np.where(k == 0, b0, edge0 + (k - 1) * FMT_WINDOW)
    stop = np.minimum(np.minimum(edge0 + k * FMT_WINDOW, b1), cap)
    lo = (addr_mod16 + b) // 16 * 16 - addr_mod16
    kind = np.where((lo >= w0) & (lo + 16 <= stop), 2, 1).astype(np.uint8)
    return kind, k


# ---- the numbers of the encoders, restated one item at a time ---------------------------------------------------------------------

def int_len(v, thresholds=INT_THRESHOLDS):
    """fmt_int_len: the bytes of std::to_string(int); thresholds: the nine steps, for the fault that moves one"""
    m = -v if v < 0 else v
    return 1 + sum(m >= t for t in thresholds) + (v < 0)


def as_int32(x):
    return x - (1 << 32) if x >= 1 << 31 else x


def gp_src(A, j, k):
    """where genotype j/k (j <= k) lies in probs' order (first allele outer, second inner)"""
    return j * (2 * A - j + 1) // 2 + (k - j)


def gp_jk(g, root=math.sqrt, drop=None):
    """(j, k) of VCF index g = k (k + 1) / 2 + j as BcfRows::put_gp finds it: a square root, put right by two loops.  root: the
    square root used; drop: 'down' or 'up' leaves one loop out (the faults)"""
    k = int((root(8.0 * g + 1.0) - 1.0) / 2.0)
    if drop != "down":
        while k * (k + 1) // 2 > g:
            k -= 1
    if drop != "up":
        while (k + 1) * (k + 2) // 2 <= g:
            k += 1
    return g - k * (k + 1) // 2, k


class Row:
    """one record: per plane gt1 / gt2 / gq, the A coverages, GP (in VCF order) with the cell's status, PL; or, for info, the
    record's slots `ac` (REF first) and `ns`"""

    def __init__(self, P=1, A=1, G=1):
        self.A, self.G = A, G
        self.gt1, self.gt2, self.gq = [0] * P, [0] * P, [0] * P
        self.cov = [[0] * A for _ in range(P)]
        self.gp = [[0.25] * G for _ in range(P)]
        self.status = [0] * P
        self.pl = [[0] * G for _ in range(P)]
        self.ac, self.ns = [], 0
        self.length = None


class TextEnc:
    name = "text"

    def __init__(self, P, haploid, fields, min_gq=None):
        self.P, self.haploid, self.fields, self.min_gq, self.keys = P, haploid, frozenset(fields), min_gq, None
        assert ("mask" in self.fields) == (min_gq is not None)

    def row(self, A=1):
        return Row(self.P, A, n_gt(A, self.haploid))

    def items(self, r):
        """-> [(kind, plane, index, bytes)] in output order"""
        out = []
        for p in range(self.P):
            out.append(("tab", p, 0, b"\t"))
            if self.min_gq is not None and r.gq[p] < self.min_gq:
                out.append(("gtmask", p, 0, b"." if self.haploid else b"./."))
            else:
                out.append(("gt1", p, 0, b"%d" % r.gt1[p]))
                if not self.haploid:
                    out += [("sep", p, 0, b"/"), ("gt2", p, 0, b"%d" % r.gt2[p])]
            out += [("sep", p, 0, b":"), ("gq", p, 0, b"%d" % r.gq[p])]
            if "COVS" in self.fields:
                if not r.A:
                    out.append(("sep", p, 0, b":"))
                for i, x in enumerate(r.cov[p]):
                    out += [("sep", p, i, b"," if i else b":"), ("covs", p, i, b"%d" % as_int32(x))]
            if "GP" in self.fields:
                out.append(("sep", p, 0, b":"))
                if r.status[p]:
                    out.append(("gpnone", p, 0, b"."))
                else:
                    for g, x in enumerate(r.gp[p]):
                        if g:
                            out.append(("sep", p, g, b","))
                        out.append(("gp", p, g, ("%.6f" % x).encode() if printable(x) else b"."))
            if "PL" in self.fields:
                out.append(("sep", p, 0, b":"))
                if all(x == PL_MISSING for x in r.pl[p]):
                    out.append(("plnone", p, 0, b"."))
                else:
                    for g, x in enumerate(r.pl[p]):
                        if g:
                            out.append(("sep", p, g, b","))
                        out.append(("pl", p, g, b"." if x == PL_MISSING else b"%d" % x))
        out.append(("nl", -1, 0, b"\n"))
        return out

    def row_len(self, r):
        if r.length is None:                                                       # (kept: a row does not change once it has been measured)
            r.length = sum(len(i[3]) for i in self.items(r))
        return r.length

    def _filler(self, digits):
        """a row whose COVS hold per plane numbers of these digit counts; no GP list, no PL value"""
        r = self.row(len(digits[0]))
        r.cov = [[10 ** (d - 1) if d > 1 else 0 for d in dp] for dp in digits]
        r.status = [1] * self.P
        r.pl = [[PL_MISSING] * r.G for _ in range(self.P)]
        return r

    def sized(self, L):
        """-> one row of exactly L bytes, or None"""
        assert "COVS" in self.fields and (self.haploid or not self.fields & {"GP", "PL"})
        P = self.P
        base = self.row_len(self._filler([[1]] * P))
        if L < base:
            return None
        per = 11 * P
        A = 1 + (L - base) // per
        digits = [[1] + [10] * (A - 1) for _ in range(P)]
        d = L - base - (A - 1) * per
        if d > 9 * P:                                                              # (one more number per plane, d - P digits together)
            for p, dp in enumerate(digits):
                dp.append((d - P) // P + (p < (d - P) % P))
            d = 0
        for dp in digits:
            for i in range(len(dp)):
                add = min(d, 10 - dp[i])
                dp[i] += add
                d -= add
        assert d == 0
        r = self._filler(digits)
        assert self.row_len(r) == L
        return r

    def fill(self, L):
        r = self.sized(L)
        return None if r is None else [r]

    def min_len(self):
        return self.row_len(self._filler([[1]] * self.P))


class InfoEnc:
    name = "info"
    P, haploid, fields, min_gq, keys = 0, True, frozenset(), None, None

    def items(self, r):
        an = sum(r.ac)
        if len(r.ac) < 2:
            return [("str", -1, 0, b"AN="), ("an", -1, 0, b"%d" % an), ("str", -1, 1, b";NS="), ("ns", -1, 0, b"%d" % r.ns)]
        out = [("str", -1, 0, b"AC=")]
        for i in range(1, len(r.ac)):
            if i > 1:
                out.append(("sep", -1, i, b","))
            out.append(("ac", -1, i, b"%d" % r.ac[i]))
        out += [("str", -1, 1, b";AN="), ("an", -1, 0, b"%d" % an), ("str", -1, 2, b";AF=")]
        for i in range(1, len(r.ac)):
            if i > 1:
                out.append(("sep", -1, i, b","))
            out.append(("af", -1, i, af_text(r.ac[i], an).encode()))
        return out + [("str", -1, 3, b";NS="), ("ns", -1, 0, b"%d" % r.ns)]

    def row_len(self, r):
        if r.length is None:                                                       # (kept: a row does not change once it has been measured)
            r.length = sum(len(i[3]) for i in self.items(r))
        return r.length

    def sized(self, L):
        r = Row()
        if L < 9:
            return None
        if L < 19:                                                                 # AN=x;NS=y
            dx = min(10, L - 8)
            r.ac, r.ns = [10 ** (dx - 1)], 10 ** (L - 7 - dx - 1)
        else:                                                                      # AC=0,0,..;AN=1;AF=0,0,..;NS=y: 4 a + 14 + digits
            a = (L - 15) // 4
            r.ac, r.ns = [1] + [0] * a, 10 ** (L - 14 - 4 * a - 1)
        assert self.row_len(r) == L
        return r

    def fill(self, L):
        r = self.sized(L)
        return None if r is None else [r]

    def min_len(self):
        return 9


class BcfEnc:
    name = "bcf"

    def __init__(self, P, haploid, fields, keys=(1, 2, 3, 4, 5), min_gq=None):
        self.P, self.haploid, self.fields, self.keys, self.min_gq = P, haploid, frozenset(fields), tuple(keys), min_gq
        assert ("mask" in self.fields) == (min_gq is not None)

    def row(self, A=1):
        return Row(self.P, A, n_gt(A, self.haploid))

    def items(self, r):
        """-> [(kind, plane, index, bytes)]: a field's header is ('hdr', -1, field, ..), its values (field, plane, index, ..)"""
        P, out = self.P, []
        masked = [self.min_gq is not None and r.gq[p] < self.min_gq for p in range(P)]

        def ints(name, key, per, cells):
            vals = [x for c in cells for x in c]
            t = int_type(min(vals), max(vals)) if vals else 1
            out.append(("hdr", -1, name, typed_int(key) + desc(per, t)))
            for p, c in enumerate(cells):
                for i, x in enumerate(c):
                    out.append((name, p, i, struct.pack(PACK[t], x)))
        ints("gt", self.keys[0], 1 if self.haploid else 2,
             [[gt_code(r.gt1[p], masked[p])] + ([] if self.haploid else [gt_code(r.gt2[p], masked[p])]) for p in range(P)])
        ints("gq", self.keys[1], 1, [[r.gq[p]] for p in range(P)])
        if "COVS" in self.fields:
            ints("covs", self.keys[2], r.A, [[as_int32(x) for x in r.cov[p]] for p in range(P)])
        if "GP" in self.fields:
            out.append(("hdr", -1, "gp", typed_int(self.keys[3]) + desc(r.G, 5)))
            for p in range(P):
                for g in range(r.G):
                    if r.status[p]:
                        f = F_EOV if g else F_MISSING
                    else:
                        x = r.gp[p][g]
                        with np.errstate(all="ignore"):
                            f = int(np.float32(x).view(np.uint32)) if printable(x) else F_MISSING
                    out.append(("gp", p, g, struct.pack("<I", f)))
        if "PL" in self.fields:
            real = [x for c in r.pl for x in c if x != PL_MISSING]
            t = int_type(min(real), max(real)) if real else 1
            out.append(("hdr", -1, "pl", typed_int(self.keys[4]) + desc(r.G, t)))
            for p in range(P):
                none = all(x == PL_MISSING for x in r.pl[p])
                for g, x in enumerate(r.pl[p]):
                    v = (PL_MISS_T[t] + (1 if none and g else 0)) if x == PL_MISSING else x
                    out.append(("pl", p, g, struct.pack(PACK[t], v)))
        return out

    def row_len(self, r):
        if r.length is None:                                                       # (kept: a row does not change once it has been measured)
            r.length = sum(len(i[3]) for i in self.items(r))
        return r.length

    def plain_len(self, A, wq=1, wt=1):
        """the bytes of a row of A alleles whose numbers are all small, but for a GQ of wq and a GT of wt bytes"""
        P, ploidy, G = self.P, 1 if self.haploid else 2, n_gt(A, self.haploid)
        n = len(typed_int(self.keys[0])) + 1 + P * ploidy * wt + len(typed_int(self.keys[1])) + 1 + P * wq
        if "COVS" in self.fields:
            n += len(typed_int(self.keys[2])) + len(desc(A, 1)) + P * A
        if "GP" in self.fields:
            n += len(typed_int(self.keys[3])) + len(desc(G, 1)) + P * G * 4
        if "PL" in self.fields:
            n += len(typed_int(self.keys[4])) + len(desc(G, 1)) + P * G
        return n

    def plain(self, A, wq=1, wt=1):
        r = self.row(A)
        r.gq[0] = {1: 0, 2: 128, 4: 40000}[wq]
        r.gt1[0] = {1: 0, 2: 63, 4: 16383}[wt]
        assert self.row_len(r) == self.plain_len(A, wq, wt)
        return r

    def _largest(self, L):
        """the most alleles of a plain row of at most L bytes"""
        lo, hi = 1, 1 << (17 if self.haploid else 11)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if self.plain_len(mid) <= L:
                lo = mid
            else:
                hi = mid - 1
        return lo

    def sized(self, L):
        """-> one row of exactly L bytes, or None"""
        for wq in (1, 2, 4):
            for wt in (1, 2, 4):
                extra = self.plain_len(1, wq, wt) - self.plain_len(1)
                if L - extra >= self.plain_len(1):
                    A = self._largest(L - extra)
                    if self.plain_len(A, wq, wt) == L:
                        return self.plain(A, wq, wt)
        return None

    def fill(self, L, max_rows=30):
        """-> rows of exactly L bytes together: plain rows, each the longest that fits, then wider GQ / GT types for the last bytes"""
        one = self.sized(L)
        if one is not None:
            return [one]
        least = self.plain_len(1)
        rows, rest = [], L
        if rest >= 7 * least:
            rows, rest = [1] * 5, rest - 5 * least
        while rest >= least and len(rows) < max_rows:
            A = self._largest(rest)
            rows.append(A)
            rest -= self.plain_len(A)
        if not rows:
            return None
        # the last `rest` bytes: per row GQ one or three bytes wider per plane, GT as much per value
        ploidy = 1 if self.haploid else 2
        reach = {0: []}
        for i in range(len(rows)):
            for which, unit in (("q", self.P), ("t", self.P * ploidy)):
                nxt = dict(reach)
                for u, how in reach.items():
                    for w, gain in ((2, unit), (4, 3 * unit)):
                        if u + gain <= rest and u + gain not in nxt:
                            nxt[u + gain] = how + [(i, which, w)]
                reach = nxt
        if rest not in reach:
            return None
        wide = {(i, which): w for i, which, w in reach[rest]}
        out = [self.plain(A, wide.get((i, "q"), 1), wide.get((i, "t"), 1)) for i, A in enumerate(rows)]
        assert sum(self.row_len(r) for r in out) == L
        return out

    def min_len(self):
        return self.plain_len(1)


# ---- a case ---------------------------------------------------------------------------------------------------------------------

class Case:
    """name; encoder 'text' | 'bcf' | 'info'; fields, a subset of COVS, GP, PL, mask; the rows (`arrays()` makes the ABI's arrays
    of them); shift: the buffer's offset in its 16-byte aligned allocation; caps: capacities below the size to cut the call at;
    seams: what the case claims to place"""

    def __init__(self, name, enc, shift, rows, seams, caps=()):
        self.name, self.enc, self.shift, self.rows, self.seams, self.caps = name, enc, shift, rows, list(seams), list(caps)
        self.encoder, self.fields, self.haploid, self.planes, self.min_gq, self.keys = enc.name, enc.fields, enc.haploid, enc.P, enc.min_gq, enc.keys
        self.n = len(rows)

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def row_off(self):
        off = np.zeros(self.n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([self.enc.row_len(r) for r in self.rows], dtype=np.uint64)
        return off

    def total(self):
        return int(self.row_off()[-1])

    def spans(self):
        """-> [(kind, plane, index, row, start, end, bytes)] over the whole output"""
        out, at = [], 0
        for v, r in enumerate(self.rows):
            for kind, p, i, b in self.enc.items(r):
                out.append((kind, p, i, v, at, at + len(b), b))
                at += len(b)
        return out

    def joined(self):
        """the output as the item spans spell it"""
        return b"".join(b for r in self.rows for _, _, _, b in self.enc.items(r))

    @functools.lru_cache(maxsize=None)
    def arrays(self):
        """-> dict of the ABI's arrays: info: ac, ns, vao; else gt1, gt2, gq [P, n] int32, cov [P, slots] uint32, vao, vgo, probs
        [P, var_gt_off[n]] in the reference's order, status, pl"""
        n, rows = self.n, self.rows
        if self.encoder == "info":
            vao = np.zeros(n + 1, dtype=np.uint32)
            vao[1:] = np.cumsum([len(r.ac) for r in rows])
            ac = np.array([x for r in rows for x in r.ac], dtype=np.uint64).astype(np.uint32)
            return dict(ac=ac, ns=np.array([r.ns for r in rows], dtype=np.uint64).astype(np.uint32), vao=vao)
        P, haploid = self.planes, self.haploid
        vao = np.zeros(n + 1, dtype=np.uint32)
        vao[1:] = np.cumsum([r.A for r in rows])
        vgo = np.zeros(n + 1, dtype=np.uint64)
        vgo[1:] = np.cumsum([r.G for r in rows])
        col = lambda name: np.array([[getattr(r, name)[p] for r in rows] for p in range(P)], dtype=np.int64).reshape(P, n)
        cov = np.array([[x for r in rows for x in r.cov[p]] for p in range(P)], dtype=np.uint64).astype(np.uint32).reshape(P, int(vao[-1]))
        pl = np.array([[x for r in rows for x in r.pl[p]] for p in range(P)], dtype=np.int64).astype(np.int32).reshape(P, int(vgo[-1]))
        probs = np.zeros((P, int(vgo[-1])), dtype=np.float64)
        for v, r in enumerate(rows):
            if haploid or r.A < 2:
                src = np.arange(r.G)
            else:
                src = np.array([gp_src(r.A, j, k) for k in range(r.A) for j in range(k + 1)], dtype=np.int64)
            for p in range(P):
                probs[p, int(vgo[v]) + src] = r.gp[p]
        return dict(gt1=col("gt1").astype(np.int32), gt2=col("gt2").astype(np.int32), gq=col("gq").astype(np.int32), cov=cov, vao=vao, vgo=vgo,
                    probs=probs, status=col("status").astype(np.uint8), pl=pl)

    @functools.lru_cache(maxsize=None)
    def expected(self):
        """-> (bytes, row_off) as the plain formatters of the existing test files make them"""
        a = self.arrays()
        if self.encoder == "info":
            from test_gpu_site_tags import info_rows
            return info_rows(a["ac"], a["ns"], a["vao"])
        f = self.fields
        cov = a["cov"] if "COVS" in f else None
        nine = (a["gt1"], a["gt2"], a["gq"], a["cov"], a["vao"], a["probs"], a["vgo"], a["status"], a["pl"])
        if self.encoder == "text":
            if "PL" in f:
                from test_gpu_pl import _rows_text
                return _rows_text(nine, self.haploid, "GP" in f, "COVS" in f, self.min_gq)
            if "GP" in f:
                from test_gpu_gp import expect_text
                return expect_text(a["gt1"], a["gt2"], a["gq"], self.haploid, a["vao"], a["probs"], a["vgo"], a["status"], cov, self.min_gq)
            if "mask" in f:
                from test_gpu_site_tags import format_masked
                return format_masked(a["gt1"], a["gt2"], a["gq"], self.haploid, self.min_gq, cov, a["vao"] if cov is not None else None)
            from test_gpu_merged import format_plain
            return format_plain(a["gt1"], a["gt2"], a["gq"], self.haploid, cov, a["vao"] if cov is not None else None)
        if "PL" in f:
            from test_gpu_pl import _rows_bcf
            return _rows_bcf(nine, self.haploid, self.keys, "GP" in f, "COVS" in f, self.min_gq)
        if "GP" in f:
            from test_gpu_gp import expect_bcf
            return expect_bcf(a["gt1"], a["gt2"], a["gq"], self.haploid, self.keys, a["vao"], a["probs"], a["vgo"], a["status"], cov, self.min_gq)
        from test_gpu_bcf import encode_plain
        return encode_plain(a["gt1"], a["gt2"], a["gq"], self.haploid, self.keys[:3], cov, a["vao"], self.min_gq)

    def second(self):
        """-> (bytes, row_off) by the second formatter of the existing tests where there is one for the case's fields, else None"""
        a = self.arrays()
        f = self.fields
        cov = a["cov"] if "COVS" in f else None
        if self.encoder == "text" and not f & {"GP", "PL", "mask"}:
            from test_gpu_merged import format_numpy
            return format_numpy(a["gt1"], a["gt2"], a["gq"], self.haploid, cov, a["vao"] if cov is not None else None)
        if self.encoder == "bcf" and not f & {"GP", "PL"}:
            from test_gpu_bcf import encode_numpy
            return encode_numpy(a["gt1"], a["gt2"], a["gq"], self.haploid, self.keys[:3], cov, a["vao"], self.min_gq)
        return None


class Build:
    """rows one behind the other; `place` opens a tile and puts an item of a row on its window's end"""

    def __init__(self, name, enc, shift=0):
        self.name, self.enc, self.shift = name, enc, shift
        self.rows, self.off, self.seams, self.caps = [], 0, [], []

    def add(self, r):
        self.rows.append(r)
        self.off += self.enc.row_len(r)

    def sized(self, L):
        r = self.enc.sized(L)
        assert r is not None, (self.name, L)
        self.add(r)

    def new_tile(self):
        while len(self.rows) % FMT_ROWS:
            self.sized(self.enc.min_len())

    def edge(self, k=0):
        """the end of window k of a tile that starts here"""
        return self.off - ((self.shift + self.off) & 15) + (k + 1) * FMT_WINDOW

    def place(self, target, pick, s, k=0, behind=None):
        """a new tile: filler rows, then `target` with the first byte of its item pick = (kind, plane, index) -- None: the byte behind
        the row -- s bytes in front of the end of the tile's window k; -> whether a filler of that length exists"""
        self.new_tile()
        items = self.enc.items(target)
        at = 0
        for kind, p, i, b in items:
            if pick is not None and (kind, p, i) == pick:
                break
            at += len(b)
        else:
            assert pick is None, (self.name, pick)
        rows = self.enc.fill(self.edge(k) - s - at - self.off)
        if rows is None:
            return False
        for r in rows + [target] + ([behind] if behind is not None else []):
            self.add(r)
        return True

    def case(self):
        return Case(self.name, self.enc, self.shift, self.rows, self.seams, self.caps)


# ---- what a seam's name means: checked on the finished case -----------------------------------------------------------------------

class Analysis:
    def __init__(self, case):
        self.case = case
        self.off = [int(x) for x in case.row_off()]
        self.total = self.off[-1]
        self.tiles = geometry(self.off, case.shift, self.total)
        self.edges = {w.w1 for t in self.tiles for w in t.windows if w.w1 < t.b1}     # where a tile goes on in a next window
        self._spans = None

    @property
    def spans(self):
        if self._spans is None:
            self._spans = self.case.spans()
        return self._spans

    def blocks(self):
        """-> [(kind, plane, start, end)]: text: a plane's cell, its tab included; bcf: a plane's values of COVS, GP or PL"""
        out, cur = [], None
        for kind, p, i, v, s, e, b in self.spans:
            if self.case.encoder == "text":
                key = ("cell", p, v) if p >= 0 else None
            else:
                key = (kind, p, v) if kind in ("covs", "gp", "pl") else None
            if cur is not None and key == cur[0]:
                cur[2] = e
            else:
                if cur is not None:
                    out.append((cur[0][0], cur[0][1], cur[1], cur[2]))
                cur = [key, s, e] if key is not None else None
        if cur is not None:
            out.append((cur[0][0], cur[0][1], cur[1], cur[2]))
        return out


@functools.lru_cache(maxsize=4)
def analysis(case):
    return Analysis(case)


INT_KINDS = {"gt": ("gt1", "gt2"), "gq": ("gq",), "covs": ("covs",), "pl": ("pl",)}
LONGEST = {"gt": b"-2147483648", "gq": b"-2147483648", "covs": b"-2147483648", "pl": b"-2147483647"}
PLANE = {"p0": lambda p, P: p == 0, "mid": lambda p, P: 0 < p < P - 1, "last": lambda p, P: p == P - 1}


def triangle(k):
    return k * (k + 1) // 2


def holds(case, seam):
    """whether the finished case has what the seam's name says, by the geometry and the item spans alone"""
    a = analysis(case)
    tiles, E, sh, n = a.tiles, a.edges, case.shift, case.n
    part = seam.split("-")
    if seam == "tile-inside-one-piece":
        t = tiles[-1]
        return 0 < t.b1 - t.b0 < 16 and (sh + t.b0) % 16 != 0 and (sh + t.b1) % 16 != 0 and (sh + t.b0) // 16 == (sh + t.b1 - 1) // 16
    if seam == "tile-on-pieces":
        return any(t.b1 > t.b0 and (sh + t.b0) % 16 == 0 and (sh + t.b1) % 16 == 0 for t in tiles)
    if seam.startswith("mis-"):
        return any(len(t.windows) >= 2 and t.windows[0].mis == int(part[1]) for t in tiles)
    if seam.startswith("window-full"):
        d = int(seam[len("window-full"):] or 0)
        return any(t.b1 - t.b0 == FMT_WINDOW - t.windows[0].mis + d for t in tiles)
    if seam == "row-ends-at-w1":
        return any(o in E for o in a.off[1:])
    if seam == "newline-first-of-window":
        return any(kind == "nl" and s in E for kind, p, i, v, s, e, b in a.spans)
    if seam == "tab-last-of-window":
        return any(kind == "tab" and e in E for kind, p, i, v, s, e, b in a.spans)
    if seam == "row-of-3-windows":
        return any(sum(w.w0 < a.off[v + 1] and w.w1 > a.off[v] for w in t.windows) >= 3 for t in tiles for v in range(t.t0, t.t1))
    if seam.startswith("cell-starts-at-w1-"):
        return any(PLANE[part[-1]](p, case.planes) and s in E for kind, p, s, e in a.blocks())
    if seam.startswith("cell-ends-at-w0-"):
        return any(PLANE[part[-1]](p, case.planes) and e in E for kind, p, s, e in a.blocks())
    if seam.startswith("int-split-"):
        return any(kind in INT_KINDS[part[3]] and b == LONGEST[part[3]] and s + int(part[2]) in E for kind, p, i, v, s, e, b in a.spans)
    if seam.startswith("gp-split-"):
        first = b"0" if part[3] == "frac" else b"1"
        return any(kind == "gp" and len(b) == 8 and b[:1] == first and s + int(part[2]) in E for kind, p, i, v, s, e, b in a.spans)
    if seam == "gp-dot-last-of-window":
        return any(kind == "gp" and b == b"." and e in E for kind, p, i, v, s, e, b in a.spans)
    if seam == "gp-dot-first-of-window":
        return any(kind == "gp" and b == b"." and s in E for kind, p, i, v, s, e, b in a.spans)
    if seam.startswith("bcf-split-"):                                               # bcf-split-<width>@<s>-<field>
        width, s_rel = (int(x) for x in part[2].split("@"))
        return any(kind == part[3] and len(b) == width and s + s_rel in E for kind, p, i, v, s, e, b in a.spans)
    if seam == "bcf-pl1-last-of-window":
        return any(kind == "pl" and len(b) == 1 and e in E for kind, p, i, v, s, e, b in a.spans)
    if seam == "bcf-pl1-first-of-window":
        return any(kind == "pl" and len(b) == 1 and s in E for kind, p, i, v, s, e, b in a.spans)
    if seam.startswith("gp-window-at-T"):                                           # gp-window-at-T<k><+d>-<dip|hap>
        k, d, mode = re.match(r"gp-window-at-T(\d+)([+-]\d)-(dip|hap)$", seam).groups()
        k, d = int(k), int(d)
        if case.haploid != (mode == "hap"):
            return False
        return any(kind == "gp" and s < w0 < e and (w0 - s) // 4 == triangle(k) + d for kind, p, s, e in a.blocks() for w0 in E)
    if seam.startswith("cap-"):
        later = [t for t in tiles if t.t0 > 0 and len(t.windows) >= 2]
        for t in later:
            b0, w1 = t.b0, t.windows[0].w1
            piece_end = b0 + 16 - (sh + b0) % 16
            ok = {"cap-at-b0": b0 in case.caps, "cap-b0+1": b0 + 1 in case.caps,
                  "cap-inside-first-piece": any(b0 + 1 < c < piece_end - 1 for c in case.caps),
                  "cap-on-piece": any(piece_end < c < w1 - 16 and (sh + c) % 16 == 0 for c in case.caps),
                  "cap-w1-1": w1 - 1 in case.caps, "cap-w1": w1 in case.caps, "cap-w1+1": w1 + 1 in case.caps,
                  "cap-in-later-window": any(w1 + 16 < c < t.b1 - 16 and (sh + c) % 16 not in (0, 15, 1) for c in case.caps)}[seam]
            if ok:
                return True
        return False
    if seam.startswith("rows-"):
        return n == int(part[1])
    if seam.startswith("records-4k+"):
        return n > 4 and n % 4 == int(seam[-1])
    if seam.startswith("desc-"):
        return case.encoder == "bcf" and case.haploid and part[2].upper() in case.fields and any(r.A == int(part[1]) for r in case.rows)
    if seam.startswith("pow10-"):
        f = part[1]
        if f in ("gt1", "gt2", "gq"):
            return {x for r in case.rows for x in getattr(r, f)} >= set(POW10)
        if f == "pl":
            return {x for r in case.rows for c in r.pl for x in c} >= set(POW10) - {PL_MISSING}
        if f == "covs":
            return {x for r in case.rows for c in r.cov for x in c} >= set(POW10_COV)
        if f == "ac":
            return {x for r in case.rows for x in r.ac[1:]} >= set(POW10_U32)
        if f == "ns":
            return {r.ns for r in case.rows} >= set(POW10_U32)
        if f == "an":
            return {sum(r.ac) for r in case.rows} >= set(POW10_AN)
    if seam.startswith("scan-n-"):
        return n == int(part[2]) and all(5 <= a.off[v + 1] - a.off[v] <= 15 for v in range(n))
    raise KeyError(seam)


# ---- which seams there are, per encoder -----------------------------------------------------------------------------------------

_GEOMETRY = (["tile-inside-one-piece", "tile-on-pieces"] + ["mis-%d" % k for k in range(16)] + ["window-full", "window-full+1", "window-full-1", "row-ends-at-w1",
             "row-of-3-windows", "cap-at-b0", "cap-b0+1", "cap-inside-first-piece", "cap-on-piece", "cap-w1-1", "cap-w1", "cap-w1+1", "cap-in-later-window",
             "rows-31", "rows-32", "rows-33", "records-4k+1", "records-4k+2", "records-4k+3"])
_CELLS = ["cell-%s-%s" % (e, p) for e in ("starts-at-w1", "ends-at-w0") for p in ("p0", "mid", "last")]
GP_WINDOW = [(1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1), (100, -1), (100, 0), (100, 1)]
REQUIRED = {
    "text": (_GEOMETRY + _CELLS + ["newline-first-of-window", "tab-last-of-window"]
             + ["int-split-%d-%s" % (s, f) for f in ("gt", "gq", "covs", "pl") for s in range(1, 11)]
             + ["gp-split-%d-%s" % (s, f) for f in ("frac", "one") for s in range(9)] + ["gp-dot-last-of-window", "gp-dot-first-of-window"]
             + ["pow10-%s" % f for f in ("gt1", "gt2", "gq", "pl", "covs")] + ["scan-n-%d" % n for n in (8191, 8192, 8193, 16385)]),
    "bcf": (_GEOMETRY + _CELLS + ["bcf-split-2@1-%s" % f for f in ("gt", "gq", "covs", "pl")]
            + ["bcf-split-4@%d-%s" % (s, f) for f in ("gt", "gq", "covs", "gp", "pl") for s in (1, 2, 3)] + ["bcf-pl1-last-of-window", "bcf-pl1-first-of-window"]
            + ["gp-window-at-T%d%+d-%s" % (k, d, m) for m in ("dip", "hap") for k, d in GP_WINDOW]
            + ["desc-%d-%s" % (n, f) for f in ("covs", "gp", "pl") for n in (14, 15, 127, 128, 32767, 32768)]),
    "info": _GEOMETRY + ["pow10-ac", "pow10-ns", "pow10-an"],
}


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def _geometry_encs():
    return [TextEnc(1, True, {"COVS"}), BcfEnc(1, True, {"COVS"}), InfoEnc()]


def _lens_case(name, enc, shift, lens, seams, caps=()):
    b = Build("%s-%s" % (enc.name, name), enc, shift)
    for L in lens:
        b.sized(L)
    b.seams, b.caps = list(seams), list(caps)
    return b.case()


def _random_row(enc, rng):
    if enc.name == "info":
        r = Row()
        r.ac = [int(x) for x in rng.integers(0, 200, size=int(rng.integers(0, 6)))]
        r.ns = int(rng.integers(0, 100))
        return r
    r = enc.row(int(rng.integers(1, 4)))
    P = enc.P
    r.gt1, r.gt2, r.gq = ([int(x) for x in rng.integers(lo, hi, size=P)] for lo, hi in ((0, 3), (0, 3), (0, 100)))
    r.cov = [[int(x) for x in rng.integers(0, 300, size=r.A)] for _ in range(P)]
    r.gp = [[float(x) for x in rng.random(size=r.G)] for _ in range(P)]
    r.status = [int(x) for x in (rng.random(size=P) < 0.2)]
    r.pl = [[int(x) for x in np.where(rng.random(size=r.G) < 0.1, PL_MISSING, rng.integers(0, 400, size=r.G))] for _ in range(P)]
    return r


def _geometry_cases():
    out = []
    for enc in _geometry_encs():
        m = enc.min_len()
        # a last tile strictly inside one 16-byte piece; a tile that is whole pieces only
        found = [(s, r, m) for s in range(16) for r in range(m, m + 16) if 1 <= (s + 31 * m + r) % 16 <= 15 - m and enc.sized(r) is not None]
        s, r, last = found[0]
        out.append(_lens_case("tile-inside-one-piece", enc, s, [m] * 31 + [r, last], ["tile-inside-one-piece", "rows-33", "records-4k+1"]))
        r = next(r for r in range(m, m + 32) if (31 * m + r) % 16 == 0 and enc.sized(r) is not None)
        out.append(_lens_case("tile-on-pieces", enc, 0, [m] * 31 + [r, 32], ["tile-on-pieces"]))
        # 16 tiles of two windows whose bytes are 1 mod 16: every misalignment once
        big = next(L for L in range(FMT_WINDOW + 40, FMT_WINDOW + 80) if (L + 31 * m) % 16 == 1 and enc.sized(L) is not None)
        out.append(_lens_case("mis-all", enc, 0, ([big] + [m] * 31) * 16, ["mis-%d" % k for k in range(16)]))
        for d in (-1, 0, 1):
            out.append(_lens_case("window-full%s" % ("%+d" % d if d else ""), enc, 3, [FMT_WINDOW - 3 + d], ["window-full%s" % ("%+d" % d if d else "")]))
        out.append(_lens_case("row-ends-at-w1", enc, 9, [FMT_WINDOW - 9, 40], ["row-ends-at-w1"]))
        out.append(_lens_case("row-of-3-windows", enc, 11, [40, 2 * FMT_WINDOW + 500, 40], ["row-of-3-windows"]))
        # the capacity on every edge of a later tile of two windows
        r = next(r for r in range(m, m + 32) if (2 + 31 * m + r) % 16 == 5 and enc.sized(r) is not None)
        b0 = 31 * m + r
        w1 = b0 - 5 + FMT_WINDOW
        out.append(_lens_case("caps", enc, 2, [m] * 31 + [r, 20000, 40], ["cap-at-b0", "cap-b0+1", "cap-inside-first-piece", "cap-on-piece", "cap-w1-1", "cap-w1",
                                                                        "cap-w1+1", "cap-in-later-window"],
                              caps=[b0, b0 + 1, b0 + 4, b0 + 11 + 160, w1 - 1, w1, w1 + 1, w1 + 1003]))
    # 31 to 34 rows of every field there is, the mask on
    for n in (31, 32, 33, 34):
        for enc in (TextEnc(3, False, {"COVS", "GP", "PL", "mask"}, 50), BcfEnc(3, False, {"COVS", "GP", "PL", "mask"}, (1, 127, 128, 32768, 200), 50), InfoEnc()):
            rng = np.random.default_rng(1000 + n)
            b = Build("%s-rows-%d" % (enc.name, n), enc, n % 16)
            for _ in range(n):
                b.add(_random_row(enc, rng))
            b.seams = (["rows-%d" % n] if n < 34 else []) + ["records-4k+%d" % (n % 4)] * (n % 4 != 0)
            out.append(b.case())
    return out


def _with(row, **kw):
    for k, v in kw.items():
        setattr(row, k, v)
    return row


def _text_cases():
    out = []
    # -2147483648 cut by the window's end behind each of its first ten bytes
    for f in ("gt", "gq", "covs", "pl"):
        enc = TextEnc(3, True, {"COVS", "PL"}) if f == "pl" else TextEnc(3, False, {"COVS"})
        b = Build("text-int-split-%s" % f, enc, 6)
        for s in range(1, 11):
            t = enc.row(3)
            plane = s % 3
            if f == "gt":
                which = "gt1" if s % 2 else "gt2"
                getattr(t, which)[plane] = INT_MIN
                pick = (which, plane, 0)
            elif f == "gq":
                t.gq[plane] = INT_MIN
                pick = ("gq", plane, 0)
            elif f == "covs":
                t.cov[plane][s % 3] = 1 << 31
                pick = ("covs", plane, s % 3)
            else:
                t.pl[plane][s % 3] = INT_MIN + 1
                pick = ("pl", plane, s % 3)
            assert b.place(t, pick, s)
            b.seams.append("int-split-%d-%s" % (s, f))
        out.append(b.case())
    # a cell that ends where a window starts, and one that starts where a window ends, per plane
    enc = TextEnc(3, True, {"COVS"})
    b = Build("text-cells", enc, 13)
    for pick, s, seams in ((("tab", 0, 0), 0, ["cell-starts-at-w1-p0", "row-ends-at-w1"]), (("tab", 1, 0), 0, ["cell-starts-at-w1-mid", "cell-ends-at-w0-p0"]),
                           (("tab", 2, 0), 0, ["cell-starts-at-w1-last", "cell-ends-at-w0-mid"]), (("nl", -1, 0), 0, ["cell-ends-at-w0-last", "newline-first-of-window"]),
                           (("tab", 1, 0), 1, ["tab-last-of-window"])):
        assert b.place(_with(enc.row(2), gq=[17, 5, 99]), pick, s)
        b.seams += seams
    out.append(b.case())
    # an 8-byte GP value cut behind each of its bytes, and a `.` on either side of the edge
    enc = TextEnc(3, True, {"COVS", "GP"})
    b = Build("text-gp-split", enc, 1)
    for name, x in (("frac", 0.123456), ("one", 1.0)):
        for s in range(9):
            t = enc.row(3)
            t.gp[1] = [0.25, x, 0.5]
            t.gp[2] = [float("nan"), 0.75, 1.0]
            assert b.place(t, ("gp", 1, 1), s)
            b.seams.append("gp-split-%d-%s" % (s, name))
    for s, seam in ((1, "gp-dot-last-of-window"), (0, "gp-dot-first-of-window")):
        t = enc.row(3)
        t.gp[1] = [0.25, float("nan"), 0.999999]
        assert b.place(t, ("gp", 1, 1), s)
        b.seams.append(seam)
    out.append(b.case())
    # every power of ten and its neighbour in every number a cell prints
    enc = TextEnc(2, False, {"COVS", "PL"})
    b = Build("text-pow10", enc, 0)
    vals = POW10 + [0]
    for j in range(len(POW10_COV)):
        t = enc.row(3)
        grab = lambda seq, k: seq[(j + k) % len(seq)]
        t.gt1, t.gt2, t.gq = [grab(vals, 0), grab(vals, 1)], [grab(vals, 2), grab(vals, 0)], [grab(vals, 1), grab(vals, 2)]
        t.cov = [[grab(POW10_COV, k) for k in range(3)], [grab(POW10_COV, k + 1) for k in range(3)]]
        t.pl = [[grab(vals, k) for k in range(6)], [grab(vals, 5 - k) for k in range(6)]]
        b.add(t)
    b.seams = ["pow10-%s" % f for f in ("gt1", "gt2", "gq", "pl", "covs")]
    out.append(b.case())
    # the scan's record counts, rows of 5 to 15 bytes
    for n in (8191, 8192, 8193, 16385):
        enc = TextEnc(1, True, set())
        rng = np.random.default_rng(n)
        b = Build("text-scan-n-%d" % n, enc, n % 16)
        for d1, d2 in zip(rng.integers(0, 6, size=n), rng.integers(0, 6, size=n)):
            b.add(_with(enc.row(0), gt1=[10 ** int(d1)], gq=[10 ** int(d2)]))
        b.seams = ["scan-n-%d" % n] + (["records-4k+%d" % (n % 4)] if n % 4 else [])
        out.append(b.case())
    return out


def _bcf_cases():
    out = []
    # a 2-byte and a 4-byte value of every field cut by the window's end; a 1-byte PL on either side of it
    enc = BcfEnc(1, True, {"COVS", "GP", "PL"}, (1, 128, 3, 32768, 5))
    b = Build("bcf-split", enc, 7)
    for f, small, big in (("gt", 63, 16383), ("gq", 128, 40000), ("covs", 300, 70000), ("pl", 300, 70000)):
        for width, s in ((2, 1), (4, 1), (4, 2), (4, 3)):
            t = enc.row(3)
            x = small if width == 2 else big
            if f == "gt":
                t.gt1[0] = x
            elif f == "gq":
                t.gq[0] = x
            else:
                getattr(t, "cov" if f == "covs" else f)[0][1] = x
            assert b.place(t, (f, 0, 0 if f in ("gt", "gq") else 1), s), (f, width, s)
            b.seams.append("bcf-split-%d@%d-%s" % (width, s, f))
    for s in (1, 2, 3):
        assert b.place(_with(enc.row(3), gp=[[0.1, 0.7, 0.2]]), ("gp", 0, 1), s)
        b.seams.append("bcf-split-4@%d-gp" % s)
    for s, seam in ((1, "bcf-pl1-last-of-window"), (0, "bcf-pl1-first-of-window")):
        assert b.place(_with(enc.row(3), pl=[[1, 7, 2]]), ("pl", 0, 1), s)
        b.seams.append(seam)
    out.append(b.case())
    # a plane's values of COVS, GP, PL starting where a window ends, and ending where one starts: one placement per case, the buffer's
    # shift chosen so that a filler of three planes has the length
    enc = BcfEnc(3, True, {"COVS", "GP", "PL"})
    nxt = {"covs": ("hdr", -1, "gp"), "gp": ("hdr", -1, "pl"), "pl": None}
    for f in ("covs", "gp", "pl"):
        for plane in (0, 1, 2, 3):
            pick = (f, plane, 0) if plane < 3 else nxt[f]
            for shift in range(16):
                b = Build("bcf-cells-%s-%s" % (f, ("p0", "mid", "last", "behind")[plane]), enc, shift)
                t = enc.row(3)
                t.cov, t.pl = [[3, 1, 4], [1, 5, 9], [2, 6, 5]], [[0, 30, 60], [30, 0, 40], [70, 20, 0]]
                t.gp = [[0.5, 0.25, 0.25], [0.1, 0.8, 0.1], [0.0, 0.0, 1.0]]
                if b.place(t, pick, 0, behind=enc.plain(1)):
                    break
            else:
                raise AssertionError("no filler for %s plane %d" % (f, plane))
            names = ("p0", "mid", "last")
            b.seams = (["cell-starts-at-w1-%s" % names[plane]] if plane < 3 else []) + (["cell-ends-at-w0-%s" % names[plane - 1]] if plane > 0 else [])
            out.append(b.case())
    # a window that starts at value T(k) - 1, T(k), T(k) + 1 of a plane's GP: T(1), T(2) in a record of 3 alleles (6 values; haploid: of
    # 6 alleles), T(100) in one of 101 alleles (5151 values; haploid: of 5060 alleles), whose values pass the end of the tile's second window
    for haploid in (False, True):
        enc = BcfEnc(1, haploid, {"COVS", "GP"})
        b = Build("bcf-gp-window-%s" % ("hap" if haploid else "dip"), enc, 4)
        for k, d in GP_WINDOW:
            g = triangle(k) + d
            t = enc.row((6 if haploid else 3) if k < 100 else (5060 if haploid else 101))
            t.gp = [[(i % 1000 + 1) / 1024.0 + (i // 1000) / 16384.0 for i in range(t.G)]]
            assert b.place(t, ("gp", 0, g), (d + 4) % 4, k=1 if k == 100 else 0), (k, d)
            b.seams.append("gp-window-at-T%d%+d-%s" % (k, d, "hap" if haploid else "dip"))
        out.append(b.case())
    # the descriptor's steps: 14 | 15 (the count moves out of the byte), 127 | 128 (int8 to int16), 32767 | 32768 (int16 to int32)
    for f in ("covs", "gp", "pl"):
        enc = BcfEnc(1, True, {f.upper()})
        b = Build("bcf-desc-%s" % f, enc, 5)
        for A in (14, 15, 127, 128, 32767, 32768):
            t = enc.row(A)
            t.cov = [[(7 * i) % 100 for i in range(A)]]
            t.gp = [[(i % 512) / 512.0 for i in range(A)]]
            t.pl = [[(3 * i) % 120 for i in range(A)]]
            b.add(t)
            b.seams.append("desc-%d-%s" % (A, f))
        out.append(b.case())
    return out


def _info_cases():
    enc = InfoEnc()
    b = Build("info-pow10", enc, 0)
    top = (1 << 32) - 1
    for i, x in enumerate(POW10_U32):
        b.add(_with(Row(), ac=[i % 3, x, POW10_U32[-1 - i]], ns=x))
    for an in POW10_AN:
        slots = []
        while an > 0:
            slots.append(min(an, top))
            an -= slots[-1]
        b.add(_with(Row(), ac=slots, ns=len(slots)))
    b.seams = ["pow10-ac", "pow10-ns", "pow10-an"]
    return [b.case()]


@functools.lru_cache(maxsize=None)
def cases():
    out = _geometry_cases() + _text_cases() + _bcf_cases() + _info_cases()
    assert len({c.name for c in out}) == len(out)
    return out


# ---- the scan (mg_debug_row_scan) -----------------------------------------------------------------------------------------------

SCAN_N = (0, 1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 16385)
U32_MAX = (1 << 32) - 1
# where the prefix passes 2^32: inside a wave, between the waves of a round, between the rounds of a part, between the parts
SCAN_SPOTS = {"inside-a-wave": 5, "between-waves": 63, "between-rounds": SCAN_TPB - 1, "between-parts": SCAN_CHUNK - 1}


def scan_model(lens, carry_bits=64):
    """-> (off[n + 1], total) in Python integers; carry_bits 32 restates the fault of a 32-bit carry in fmt_rescan_kernel: what a
    workgroup carries from round to round, its part's start included, is cut to 32 bits"""
    mask = (1 << carry_bits) - 1
    off, total = [], 0
    for base in range(0, len(lens), SCAN_CHUNK):
        carry = total & mask
        for r0 in range(base, min(base + SCAN_CHUNK, len(lens)), SCAN_TPB):
            run = 0
            for x in lens[r0:r0 + SCAN_TPB]:
                off.append(carry + run)
                run += int(x)
            carry = (carry + run) & mask
        total += sum(int(x) for x in lens[base:base + SCAN_CHUNK])
    return off + [carry if len(lens) else 0], total


def scan_inputs(n):
    """-> [(name, lens)] for a record count: all 0xFFFFFFFF, one 0xFFFFFFFF among zeros at each spot there is, seeded random"""
    out = [("all-max", np.full(n, U32_MAX, dtype=np.uint32))]
    for name, at in SCAN_SPOTS.items():
        if at < n:
            x = np.zeros(n, dtype=np.uint32)
            x[at] = U32_MAX
            if at + 1 < n:
                x[at + 1] = 1                                                       # (the sum passes 2^32 behind the spot)
            out.append(("one-max-%s" % name, x))
    out.append(("random", np.random.default_rng(n).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)))
    return out
