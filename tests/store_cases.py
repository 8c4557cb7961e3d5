"""Directed cases for the two stores underneath everything (csrc/store_kernels.h, csrc/kmer_dev.h): the Bloom filter's bits, its
rank directory and u16 counters, the directory's copy inside the exact map's records, the exact map, and sparse import.  No GPU
and no product import here: tests/test_store_cases_cpu.py checks on any machine that every case holds what its name says and that
the numpy model below agrees with the oracle; tests/test_gpu_store_edges.py hands the same cases to the device.

The seams the tables aim at (the formulas are mg_create's and mg_bf_finalize's):
    nwords = ceil(size / 64), n_blk = ceil(nwords / 8)          512-bit blocks; blk[n_blk] holds the total
    n_tiles = ceil((n_blk + 1) / 256)                           blk_pop_kernel: one workgroup per tile of TPB = 256 blocks
    n_part = ceil(n_tiles / 8192)                               launch_tile_scan: chunks of SCAN_CHUNK tile sums (2^30 bits);
                                                                inside a chunk, rounds of 1,024 sums and waves of 64
mg_create accepts every size >= 1 and every k in 1..128 (ref_k >= k), so no size or k below is replaced by a larger one.

Filter patterns are ascending positions.  "directed blocks" of a size are the blocks on either side of every tile seam the table
names for it (block 256 m - 1 and 256 m), and the filter's last block."""
import functools
import os
from collections import namedtuple

import numpy as np

from oracle import capi as ocapi

TPB, BLOCK_BITS, SCAN_TPB, SCAN_CHUNK = 256, 512, 1024, 8192
TILE_BITS = TPB * BLOCK_BITS                 # 131,072
CHUNK_BITS = SCAN_CHUNK * TILE_BITS          # 2^30
MAX_PACKED_K, MAX_KMER = 64, 128
K = 35

SMALL_SIZES = [64, 65, 511, 512, 513, 4099]
TILE_SIZES = [130560, 131071, 131072, 131073, 3 * TILE_BITS + 77]
CHUNK_SIZES = [CHUNK_BITS - 512, CHUNK_BITS, CHUNK_BITS + 3 * TILE_BITS + 77]
SIZES = SMALL_SIZES + TILE_SIZES + CHUNK_SIZES
# tile seams (in tiles) aimed at where the filter has 8,192 of them: the scan's waves (64), its rounds (1,024) and the chunk
CHUNK_SEAM_TILES = [1, 63, 64, 65, 1023, 1024, 1025, 4096, 8191, 8192, 8193, 8194, 8195]


def geometry(size):
    nwords = (size + 63) // 64
    n_blk = (nwords + 7) // 8
    n_tiles = (n_blk + 1 + TPB - 1) // TPB
    n_part = (n_tiles + SCAN_CHUNK - 1) // SCAN_CHUNK
    return nwords, n_blk, n_tiles, n_part


def seam_tiles(size):
    """the tile seams m (block 256 m starts a tile, or is the total's entry) the table aims at for this size"""
    n_blk = geometry(size)[1]
    every = range(1, n_blk // TPB + 1)
    return [m for m in (CHUNK_SEAM_TILES if size >= CHUNK_BITS - 512 else every) if m * TPB <= n_blk]


def directed_blocks(size):
    n_blk = geometry(size)[1]
    blocks = {n_blk - 1}
    for m in seam_tiles(size):
        blocks.update(b for b in (m * TPB - 1, m * TPB) if b < n_blk)
    return sorted(blocks)


def outer_neighbours(size):
    """the blocks next to the directed ones that are not directed themselves: they stay empty in the `full` pattern"""
    n_blk, d = geometry(size)[1], set(directed_blocks(size))
    return sorted({b for x in d for b in (x - 1, x + 1) if 0 <= b < n_blk and b not in d})


def block_bits(size, b):
    return np.arange(b * BLOCK_BITS, min((b + 1) * BLOCK_BITS, size), dtype=np.uint64)


# ---- k-mers and the oracle's hash -------------------------------------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def random_kmers(seed, n, k):
    rng = np.random.default_rng(seed)
    return [bytes(r) for r in _ACGT[rng.integers(0, 4, size=(n, k))]]


def revcomp(km):
    return km[::-1].translate(_COMP)


def hashes(kmers):
    """BF::_get_hash of each k-mer, from the oracle (never from the device)"""
    f = ocapi.lib().mo_bf_hash
    return np.array([f(km) for km in kmers], dtype=np.uint64)


POOL_N = 40000


@functools.lru_cache(maxsize=None)
def pool():
    """the probing k-mers every filter case draws from, hashed once: slot = hash % size"""
    kmers = random_kmers(20240, POOL_N, K)
    return kmers, hashes(kmers)


DEEP_N = 400000


@functools.lru_cache(maxsize=None)
def deep_pool():
    """ten times as many, for trailing blocks too narrow for the pool: the 77 bits of 3 * 131,072 + 77 (expected there: 78 of these)"""
    kmers = random_kmers(20241, DEEP_N, K)
    return kmers, hashes(kmers)


SLOT_SIZE, SLOT, SLOT_SEED = 131073, 131072, 131073000
SLOT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "store_slot_131072_kmers.txt")


def find_slot_kmers(n=24):
    """how SLOT_FILE was made (4 s: 2.8 million hashes): the first n seeded 35-mers whose slot at size 131,073 is its last bit, the
    single bit of the first block behind the tile seam.  tests/test_store_cases_cpu.py holds the file to this search's first batches
    only through the hashes: every k-mer of the file must hash to the slot."""
    found, seed = [], SLOT_SEED
    while len(found) < n:
        kmers = random_kmers(seed, 200000, K)
        found += [kmers[i] for i in np.flatnonzero(hashes(kmers) % np.uint64(SLOT_SIZE) == SLOT)]
        seed += 1
    return found[:n]


@functools.lru_cache(maxsize=None)
def slot_kmers():
    kmers = [line.strip().encode() for line in open(SLOT_FILE) if line.strip()]
    return kmers, hashes(kmers)


# ---- filter cases -----------------------------------------------------------------------------------------------------------
PATTERNS = ["empty", "bit0", "bitlast", "allones", "altwords", "edges", "full"]
PER_BLOCK, EXTRA = 24, 300                     # probing k-mers kept per directed block, and others on top
FilterCase = namedtuple("FilterCase", "name size pattern pos counts probe probe_idx inc hits")


def patterns_of(size):
    return [p for p in PATTERNS if p != "allones" or size <= 131073]


def filter_case_ids():
    return ["%d-%s" % (s, p) for s in SIZES for p in patterns_of(s)]


def counts_of(n):
    """counter of rank r: swapping any two ranks changes an answer"""
    return ((np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(1)) & np.uint64(0xFFFF)).astype(np.uint16)


def _probe_pick(size):
    """(k-mers, their hashes, {directed block: how many fall in it}): up to PER_BLOCK k-mers per directed block, then EXTRA
    others (some of them twice: they meet again at their slot, like k-mers of different text that merely collide there).
    A trailing block of a few bits that the pool misses draws on the deep pool, the one-bit block of 131,073 on the recorded search."""
    kmers, h = pool()
    blk = ((h % np.uint64(size)) // np.uint64(BLOCK_BITS)).astype(np.int64)
    out_k, out_h, per_block = [], [], {}
    for b in directed_blocks(size):
        got = np.flatnonzero(blk == b)[:PER_BLOCK]
        out_k += [kmers[i] for i in got]
        out_h += [h[i] for i in got]
        if len(got) < PER_BLOCK and size < CHUNK_BITS - 512:
            dk, dh = slot_kmers() if (size, b) == (SLOT_SIZE, SLOT // BLOCK_BITS) else deep_pool()
            more = np.flatnonzero(((dh % np.uint64(size)) // np.uint64(BLOCK_BITS)).astype(np.int64) == b)[:PER_BLOCK - len(got)]
            out_k += [dk[i] for i in more]
            out_h += [dh[i] for i in more]
            got = np.concatenate([got, more])
        per_block[b] = len(got)
    others = list(range(EXTRA)) + list(range(0, EXTRA, 7))
    out_k += [kmers[i] for i in others]
    out_h += [h[i] for i in others]
    return out_k, np.array(out_h, dtype=np.uint64), per_block


def _pattern_positions(size, pattern, probe_idx):
    nwords = geometry(size)[0]
    big = size >= CHUNK_BITS - 512
    if pattern == "empty":
        pos = np.zeros(0, dtype=np.uint64)
    elif pattern == "bit0":
        pos = np.array([0], dtype=np.uint64)
    elif pattern == "bitlast":
        pos = np.array([size - 1], dtype=np.uint64)
    elif pattern == "allones":
        pos = np.arange(size, dtype=np.uint64)
    elif pattern == "altwords":
        # every even word all ones; at the 2^30 sizes (2^29 positions otherwise) only inside the directed blocks and their neighbours
        if big:
            blocks = sorted(set(directed_blocks(size)) | set(outer_neighbours(size)))
            words = np.concatenate([np.arange(b * 8, min(b * 8 + 8, nwords), 2) for b in blocks])
        else:
            words = np.arange(0, nwords, 2)
        pos = (words[:, None].astype(np.uint64) * np.uint64(64) + np.arange(64, dtype=np.uint64)[None, :]).ravel()
        pos = pos[pos < size]
    elif pattern == "edges":
        pos = np.array(sorted({int(x) for b in directed_blocks(size) for x in (block_bits(size, b)[0], block_bits(size, b)[-1])}), dtype=np.uint64)
    elif pattern == "full":
        pos = np.concatenate([block_bits(size, b) for b in directed_blocks(size)])
    else:
        raise KeyError(pattern)
    if big and pattern != "empty":
        # 20,000 seeded random positions on top of the directed ones, and the probing k-mers' own slots, so that hits exist
        rng = np.random.default_rng(size % 1000 + len(pattern))
        more = np.concatenate([rng.integers(0, size, size=20000, dtype=np.uint64), probe_idx[::2]])
        if pattern == "full":                                  # (the directed blocks' neighbours stay empty)
            more = more[~np.isin(more // np.uint64(BLOCK_BITS), np.array(outer_neighbours(size), dtype=np.uint64))]
        pos = np.concatenate([pos, more])
    return np.unique(pos).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def filter_case(name):
    size, pattern = name.split("-")
    size = int(size)
    probe, probe_h, _ = _probe_pick(size)
    probe_idx = probe_h % np.uint64(size)
    pos = _pattern_positions(size, pattern, probe_idx)
    rng = np.random.default_rng(len(pos) + size % 977)
    inc = rng.integers(1, 70000, size=len(probe)).astype(np.uint32)     # (beyond 65,535: a cell wraps on one addition, and on sums)
    hits = int(np.isin(probe_idx, pos).sum())
    return FilterCase(name, size, pattern, pos, counts_of(len(pos)), probe, probe_idx, inc, hits)


def words_of(size, pos):
    w = np.zeros(geometry(size)[0], dtype=np.uint64)
    np.bitwise_or.at(w, (pos >> np.uint64(6)).astype(np.int64), np.uint64(1) << (pos & np.uint64(63)))
    return w


class FilterModel:
    """rank = index in the sorted positions, counters by rank (u16, wrapping)"""

    def __init__(self, pos, counts):
        self.pos = np.asarray(pos, dtype=np.uint64)
        self.counts = np.array(counts, dtype=np.uint16)

    def rank(self, idx):
        """(rank, hit) of slots"""
        idx = np.asarray(idx, dtype=np.uint64)
        r = np.searchsorted(self.pos, idx)
        hit = np.zeros(len(idx), dtype=bool)
        inside = r < len(self.pos)
        hit[inside] = self.pos[r[inside]] == idx[inside]
        return r, hit

    def increment(self, idx, c):
        r, hit = self.rank(idx)
        acc = self.counts.astype(np.uint64)
        np.add.at(acc, r[hit], np.asarray(c, dtype=np.uint64)[hit])
        self.counts = (acc & np.uint64(0xFFFF)).astype(np.uint16)

    def get_count(self, idx):
        r, hit = self.rank(idx)
        out = np.zeros(len(r), dtype=np.uint16)
        out[hit] = self.counts[r[hit]]
        return out


def oracle_filter(size, pos, counts):
    """the oracle's filter holding exactly these bits and counters, in read mode"""
    obf = ocapi.BF(size)
    obf.load_words(words_of(size, pos))
    obf.switch_mode()
    if len(pos):
        obf.counts()[:] = counts
    return obf


# ---- scan cases (mg_debug_tile_scan) ----------------------------------------------------------------------------------------
SCAN_NS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 8388607, 8388608, 8388609, 8388608 + 8192 + 3]
SINGLE_NS = [8193, 8388608 + 8192 + 3]                         # a chunk seam, and the second round's seam, inside
SINGLE_AT = [0, 63, 64, 1023, 1024, 8191, 8192, 8388607, 8388608, -1]
BIG_SCAN = "big-40000x131072"


def scan_case_ids():
    ids = ["ones-%d" % n for n in SCAN_NS] + ["random-%d" % n for n in SCAN_NS]
    for n in SINGLE_NS:
        ids += ["single-%d-at-%d" % (n, a) for a in sorted({a % n for a in SINGLE_AT if a < n})]
    return ids + [BIG_SCAN]


def scan_values(name):
    if name == BIG_SCAN:
        return np.full(40000, 131072, dtype=np.uint32)          # total 5,242,880,000
    kind, rest = name.split("-", 1)
    if kind == "ones":
        return np.ones(int(rest), dtype=np.uint32)
    if kind == "random":
        n = int(rest)
        return np.random.default_rng(n % 9973).integers(0, 131073, size=n, dtype=np.uint32)
    n, _, at = rest.split("-")
    x = np.zeros(int(n), dtype=np.uint32)
    x[int(at)] = 131072
    return x


def scan_model(x):
    """(exclusive prefix, total) in uint64"""
    inc = np.cumsum(x.astype(np.uint64), dtype=np.uint64)
    return inc - x.astype(np.uint64), int(inc[-1]) if len(x) else 0


# ---- the directory inside the records ---------------------------------------------------------------------------------------
GOLDEN_MUL = 0x9E3779B97F4A7C15
DIR_SIZE = 1 << 20
DirCase = namedtuple("DirCase", "name size pos counts keys_before keys_after probe probe_idx inc")


def home_mul(size, ordered):
    return (2 ** 64 - 1) // size if ordered else GOLDEN_MUL


def home(idx, size, cap_log2, ordered):
    """map_home: the record a filter slot starts its walk at"""
    return ((np.asarray(idx, dtype=np.uint64) * np.uint64(home_mul(size, ordered))) >> np.uint64(64 - cap_log2)).astype(np.int64)


def table_log2(rows, nset):
    """map_reserve: the smallest table (>= 2^10 records) with key load <= 1/4 and two directory entries per record at load <= 1/4"""
    want = 10
    while (1 << want) < rows * 4 or (1 << want) < nset * 2:
        want += 1
    return want


def _pool_slots(n):
    """the first n distinct slots of the pool's k-mers at DIR_SIZE: set bits that probing k-mers hit"""
    seen = []
    have = set()
    for i in (pool()[1] % np.uint64(DIR_SIZE)).tolist():
        if i not in have:
            have.add(i)
            seen.append(i)
            if len(seen) == n:
                break
    return np.array(sorted(seen), dtype=np.uint64)


def _dir_pos(name):
    if name == "nset-512":
        return DIR_SIZE, _pool_slots(512)
    if name in ("nset-513", "keys-after", "keys-before"):
        return DIR_SIZE, _pool_slots(513)
    if name == "run-600":            # 2^11 records of 512 slots each; home_mul rounds down, so record r is the home of slots 512 r + 1 ..
        return DIR_SIZE, np.arange(512 * 1000 + 1, 512 * 1000 + 601, dtype=np.uint64)    # 512 r + 512: 512 of the 600 share one home
    if name == "run-600-end":        # ends at size - 1: the chain leaves the last record and goes on at record 0
        return DIR_SIZE, np.arange(DIR_SIZE - 600, DIR_SIZE, dtype=np.uint64)
    if name == "run-600-4099":       # two entries per record and two slots per record, but for three records of three (0, 682, 1365): the
        return 4099, np.arange(2732, 3332, dtype=np.uint64)     # run starts at 1365's first slot, whose third bit is pushed past 299 full records
    raise KeyError(name)


DIR_CASES = ["nset-512", "nset-513", "run-600", "run-600-end", "run-600-4099", "keys-after", "keys-before"]
DIR_KEYS = 3000


@functools.lru_cache(maxsize=None)
def dir_case(name):
    size, pos = _dir_pos(name)
    kmers, h = pool()
    idx = h % np.uint64(size)
    pick = np.concatenate([np.flatnonzero(np.isin(idx, pos))[:600], np.flatnonzero(~np.isin(idx, pos))[:200]])
    inc = np.random.default_rng(len(pick)).integers(1, 70000, size=len(pick)).astype(np.uint32)
    before = random_kmers(51, DIR_KEYS, K) if name == "keys-before" else []
    return DirCase(name, size, pos, counts_of(len(pos)), before, random_kmers(52, DIR_KEYS, K),      # (every case ends with the later insert that rehashes)
                   [kmers[i] for i in pick], idx[pick], inc)


# ---- exact map --------------------------------------------------------------------------------------------------------------
MAP_KS = [1, 31, 32, 33, 63, 64, 65, 128]                      # 1: the smallest k mg_create accepts
IUPAC = b"NaW"                                                 # N, a lower-case letter, an IUPAC code
MapCase = namedtuple("MapCase", "k rows groups")


def lform(km):
    """L-form halves of a pure-ACGT string of <= 64 bases: base i at bits 2i of lo (i < 32) or 2(i - 32) of hi"""
    lo = hi = 0
    for i, ch in enumerate(km):
        code = b"ACGT".index(ch)
        if i < 32:
            lo |= code << (2 * i)
        else:
            hi |= code << (2 * (i - 32))
    return lo, hi


def is_regular(km, k):
    return len(km) == k and k <= MAX_PACKED_K and all(ch in b"ACGT" for ch in km)


def canonical_key(km):
    """the key KMAP files a k-mer under (kmap.hpp:86-97), read off the oracle's map"""
    om = ocapi.KMAP()
    om.add_key(km)
    return next(iter(om.items()))[0]


def _with(km, i, ch):
    return km[:i] + bytes([ch]) + km[i + 1:]


@functools.lru_cache(maxsize=None)
def map_case(k):
    """rows of one k, by group.  Keys that must keep their orientation start and end with A: the reverse complement then starts
    with T, so the text itself is the canonical form and the named base sits where the name says."""
    g = {}
    g["random"] = random_kmers(100 + k, 60, k)
    g["revcomp"] = [revcomp(km) for km in g["random"][:20]]
    if k % 2 == 0:
        g["palindrome"] = [h + revcomp(h) for h in random_kmers(200 + k, 5, k // 2)]
    g["all-A-all-T"] = [b"A" * k, b"T" * k]
    anchored = [_with(_with(km, 0, 65), k - 1, 65) for km in random_kmers(300 + k, 4, k)]
    bases = sorted({i for i in (0, 31, 32, k - 1) if i < k})
    for i in bases:
        tag = "last" if i == k - 1 else str(i)
        others = b"ACG" if i in (0, k - 1) else b"ACGT"        # (an end base stays off T: the text stays canonical)
        if k == 1:
            others = b"AC"
        g["differ-at-%s" % tag] = [_with(km, i, ch) for km in anchored for ch in others]
        g["irregular-at-%s" % tag] = [_with(km, i, ch) for km in anchored[:2] for ch in IUPAC]
    if k > 1:
        g["length-k-1"] = [km[:-1] for km in anchored]
    if k + 1 <= MAX_KMER:                                      # (a row holds at most MG_MAX_KMER bytes: no k + 1 at k = 128)
        g["length-k+1"] = [km + b"C" for km in anchored]
    rows = [km for name in g for km in g[name]]
    return MapCase(k, rows, g)


def stride_k_rows(k):
    """rows that fill their stride exactly, no terminator"""
    keys = random_kmers(400 + k, 16, k)
    return keys, np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), k).copy()


GROWTH_BATCHES = [200, 1000, 5000, 25000, 125000]          # (the first fits the table as created: the fifth makes it four growths)
WRAP_SIZE, WRAP_TRIES = 4099, 200000


@functools.lru_cache(maxsize=None)
def wrap_keys():
    """35-mers whose filter slot at size 4099 is size - 1 or size - 2: under the ordered home they all start at the last record"""
    kmers = random_kmers(4099, WRAP_TRIES, K)
    idx = hashes(kmers) % np.uint64(WRAP_SIZE)
    keep = np.flatnonzero(idx >= WRAP_SIZE - 2)
    return [kmers[i] for i in keep], idx[keep]


# ---- sparse import ----------------------------------------------------------------------------------------------------------
SPARSE_SIZE, SPARSE_N = 4099, 600


def sparse_clean():
    return np.arange(SPARSE_N, dtype=np.uint64) * np.uint64(5) + np.uint64(3)


def _pair(i, kind):
    def make():
        p = sparse_clean()
        p[i + 1] = p[i] if kind == "equal" else p[i] - np.uint64(1)
        return p
    return make


def _beyond(i):
    def make():
        p = sparse_clean() if i < 0 else sparse_clean()[: i + 1]
        p[i] = SPARSE_SIZE
        return p
    return make


SPARSE_REFUSALS = {"%s-%d-%d" % (kind, i, i + 1): _pair(i, kind) for i in (254, 255, 256) for kind in ("equal", "descending")}
SPARSE_REFUSALS["size-as-last"] = _beyond(-1)
SPARSE_REFUSALS["size-at-256"] = _beyond(256)
