"""tests/store_cases.py holds what its names say, and its numpy model agrees with the oracle -- checked from the tables alone, on
any machine.  Nothing here is skipped or filtered at run time: a case the table cannot realise fails."""
import numpy as np
import pytest

import store_cases as sc
from oracle import capi as ocapi


# ---- geometry: the named seams are exactly met --------------------------------------------------------------------------------
def test_sizes_sit_on_the_seams_they_name():
    g = {s: sc.geometry(s) for s in sc.SIZES}
    assert [g[s][1] for s in sc.SMALL_SIZES] == [1, 1, 1, 1, 2, 9] and all(g[s][2] == 1 for s in sc.SMALL_SIZES)
    # around one tile: the total's entry blk[n_blk] is the tile's last thread (255), a tile of its own (256), or shares the second (257)
    assert g[130560][1:3] == (255, 1) and (g[130560][1] + 1) % sc.TPB == 0
    assert g[131071][1:3] == (256, 2) and g[131072][1:3] == (256, 2) and g[131072][1] % sc.TPB == 0
    assert g[131073][1:3] == (257, 2)
    assert g[3 * sc.TILE_BITS + 77][1:3] == (769, 4) and (3 * sc.TILE_BITS + 77) % 64 != 0
    # around one chunk of the tile scan: exactly full, one tile more (the total's, alone in chunk 1), and a ragged second chunk
    assert g[sc.CHUNK_BITS - 512][2:] == (sc.SCAN_CHUNK, 1)
    assert g[sc.CHUNK_BITS][1:] == (1 << 21, sc.SCAN_CHUNK + 1, 2) and g[sc.CHUNK_BITS][1] % sc.TPB == 0
    assert g[sc.CHUNK_BITS + 3 * sc.TILE_BITS + 77][2:] == (sc.SCAN_CHUNK + 4, 2)
    for s in sc.CHUNK_SIZES:                                   # the seams named there exist: waves, rounds and the chunk of the scan
        assert {63, 64, 65, 1023, 1024, 1025, 8191}.issubset(sc.seam_tiles(s))
    assert 8192 in sc.seam_tiles(sc.CHUNK_BITS) and 8195 in sc.seam_tiles(sc.CHUNK_SIZES[2]) and 8192 not in sc.seam_tiles(sc.CHUNK_SIZES[0])
    for s in sc.TILE_SIZES[1:]:
        assert sc.seam_tiles(s) == list(range(1, g[s][1] // sc.TPB + 1)) and sc.seam_tiles(s)
    assert sc.seam_tiles(130560) == [] and sc.directed_blocks(130560) == [254]


def test_scan_sizes_sit_on_the_scan_seams():
    ns = sc.SCAN_NS
    for seam in (64, sc.SCAN_TPB, sc.SCAN_CHUNK, sc.SCAN_TPB * sc.SCAN_CHUNK):     # wave, round, chunk, part_scan_kernel's second round
        assert {seam - 1, seam, seam + 1}.issubset(ns)
    assert 0 in ns and 1 in ns and 2 * sc.SCAN_CHUNK in ns and ns[-1] == sc.SCAN_TPB * sc.SCAN_CHUNK + sc.SCAN_CHUNK + 3
    assert (ns[-1] + sc.SCAN_CHUNK - 1) // sc.SCAN_CHUNK == sc.SCAN_TPB + 2        # two chunk totals in the second round
    ids = sc.scan_case_ids()
    assert len(ids) == len(set(ids))
    big = sc.scan_values(sc.BIG_SCAN)
    assert sc.scan_model(big)[1] == 5242880000 > 1 << 32
    for name in ids:
        if name.startswith("single"):
            x = sc.scan_values(name)
            assert np.count_nonzero(x) == 1 and len(x) in sc.SINGLE_NS
    for n in sc.SINGLE_NS:
        at = {int(name.rsplit("-", 1)[1]) for name in ids if name.startswith("single-%d-" % n)}
        assert {0, n - 1}.issubset(at) and {a for a in (8191, 8192) if a < n}.issubset(at)
    assert {8388607, 8388608}.issubset({int(name.rsplit("-", 1)[1]) for name in ids if name.startswith("single-%d-" % sc.SINGLE_NS[1])})
    assert sc.scan_model(sc.scan_values("random-8388609"))[1] > 1 << 32             # the carry into the second round is beyond 32 bits


# ---- filter cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.filter_case_ids())
def test_filter_case(name):
    c = sc.filter_case(name)
    size, pos = c.size, c.pos
    nwords, n_blk, n_tiles, n_part = sc.geometry(size)
    big = size in sc.CHUNK_SIZES
    assert pos.dtype == np.uint64 and (len(pos) == 0 or (np.all(np.diff(pos.astype(np.int64)) > 0) and int(pos[-1]) < size))
    assert len(c.counts) == len(pos) and len(c.probe) == len(c.probe_idx) == len(c.inc)
    assert np.array_equal(c.probe_idx, sc.hashes(c.probe) % np.uint64(size))
    if len(pos) > 1:
        assert c.counts[0] != c.counts[1] and len(set(c.counts[:64].tolist())) == min(64, len(pos))   # swapping ranks shows
    per_block = np.bincount((pos // np.uint64(sc.BLOCK_BITS)).astype(np.int64), minlength=n_blk)
    width = np.array([len(sc.block_bits(size, b)) for b in sc.directed_blocks(size)])
    d = np.array(sc.directed_blocks(size))
    if c.pattern == "empty":
        assert len(pos) == 0
    if c.pattern == "bit0" and not big:
        assert pos.tolist() == [0]
    if c.pattern == "bitlast" and not big:
        assert pos.tolist() == [size - 1]
    if c.pattern in ("bit0", "bitlast"):
        assert (0 if c.pattern == "bit0" else size - 1) in pos
    if c.pattern == "allones":
        assert len(pos) == size
    if c.pattern == "altwords" and not big:
        w = sc.words_of(size, pos)
        assert np.all(w[1::2] == 0) and np.all(w[0:-1:2] == np.uint64(0xFFFFFFFFFFFFFFFF)) and len(pos) > 0
    if c.pattern == "edges":                                   # the first and last bit of every directed block: bits on both sides of every seam
        for b in d:
            bits = sc.block_bits(size, b)
            assert bits[0] in pos and bits[-1] in pos
        if not big:
            assert np.array_equal(per_block[d], np.minimum(width, 2)) and per_block.sum() == per_block[d].sum()
    if c.pattern == "full":                                    # which blocks are full: the directed ones, and their neighbours are empty
        assert np.array_equal(per_block[d], width)
        assert not per_block[sc.outer_neighbours(size)].any()
        if not big:
            assert per_block.sum() == width.sum()
    for m in sc.seam_tiles(size):                              # set bits on both sides of every seam named
        if c.pattern in ("edges", "full", "allones", "altwords") and m * sc.TPB < n_blk:
            assert per_block[m * sc.TPB - 1] > 0 and per_block[m * sc.TPB] > 0, m
    if big and c.pattern != "empty":
        assert len(pos) >= 20000 and c.hits >= len(c.probe) // 2   # random positions on top, and the probing k-mers' own slots
    # probing k-mers: at least 20 in every directed block (which the full pattern fills)
    if not big:
        _, _, got = sc._probe_pick(size)
        for b in d:
            assert got[b] >= 20, (b, got[b])
        if c.pattern == "full":
            assert c.hits >= 20 * len(d)
            blk_of = (c.probe_idx // np.uint64(sc.BLOCK_BITS)).astype(np.int64)
            assert all((blk_of == b).sum() >= 20 for b in d)
    assert len(set(c.probe)) < len(c.probe)                    # some k-mers come twice
    assert (c.inc > 65535).any()
    if c.hits >= 20:                                           # a cell wraps on the way
        r, hit = sc.FilterModel(pos, c.counts).rank(c.probe_idx)
        acc = c.counts.astype(np.int64)
        np.add.at(acc, r[hit], c.inc[hit].astype(np.int64))
        assert (acc > 65535).any()
    if size >= sc.CHUNK_BITS:
        return
    # every case below 2^30: the model against the oracle, loaded from the same words: positions, ranks through the counters, increments, wrap-around
    obf = sc.oracle_filter(size, pos, c.counts)
    model = sc.FilterModel(pos, c.counts)
    assert obf.nset == len(pos) and np.array_equal(obf.set_positions(), pos)
    assert np.array_equal(model.get_count(c.probe_idx), np.array([obf.get_count(km) for km in c.probe], dtype=np.uint16))
    for km, n in zip(c.probe, c.inc):
        assert obf.increment(km, int(n))
    model.increment(c.probe_idx, c.inc)
    assert np.array_equal(model.counts, obf.counts())
    assert np.array_equal(model.get_count(c.probe_idx), np.array([obf.get_count(km) for km in c.probe], dtype=np.uint16))


def test_every_size_has_every_pattern():
    ids = sc.filter_case_ids()
    assert len(ids) == len(set(ids)) == 7 * 10 + 6 * 4
    for s in sc.SIZES:
        assert ("%d-allones" % s in ids) == (s <= 131073)


# ---- scan model -----------------------------------------------------------------------------------------------------------------
def test_scan_model_is_an_exclusive_scan_in_64_bits():
    x = np.array([3, 0, 0xFFFFFFFF, 0xFFFFFFFF, 5], dtype=np.uint32)
    pre, total = sc.scan_model(x)
    assert pre.tolist() == [0, 3, 3, 3 + 0xFFFFFFFF, 3 + 2 * 0xFFFFFFFF] and total == 8 + 2 * 0xFFFFFFFF
    assert sc.scan_model(np.zeros(0, np.uint32))[1] == 0


# ---- directory cases ------------------------------------------------------------------------------------------------------------
def test_directory_cases_cross_what_they_name():
    a, b = sc.dir_case("nset-512"), sc.dir_case("nset-513")
    assert len(a.pos) == 512 and len(b.pos) == 513                                  # the position count crosses 512 ...
    assert sc.table_log2(0, 512) == 10 and sc.table_log2(0, 513) == 11              # ... and the directory alone grows the table
    for name in sc.DIR_CASES:
        c = sc.dir_case(name)
        assert np.all(np.diff(c.pos.astype(np.int64)) > 0) and int(c.pos[-1]) < c.size
        before = sc.table_log2(len(c.keys_before), len(c.pos))
        after = sc.table_log2(len(c.keys_before) + len(c.keys_after), len(c.pos))
        assert after > before, name                                                 # the later insert rehashes and rewrites the directory
        assert len(set(c.keys_after) | set(c.keys_before)) == len(c.keys_after) + len(c.keys_before)
        hit = np.isin(c.probe_idx, c.pos)
        assert hit.sum() >= 20 and (~hit).sum() == 200 and np.array_equal(c.probe_idx, sc.hashes(c.probe) % np.uint64(c.size))
    assert len(sc.dir_case("keys-before").keys_before) == 3000 and len(sc.dir_case("keys-after").keys_after) == 3000
    assert sc.table_log2(3000, 513) == 14 > sc.table_log2(0, 513)
    # the run: one ordered home for 512 of the 600 (a record of the 2^11-record table spans 512 slots, so 600 cannot share one),
    # a chain of 300 records
    run = sc.dir_case("run-600")
    assert len(run.pos) == 600 and int(run.pos[0]) % 512 == 1 and int(run.pos[-1]) - int(run.pos[0]) == 599
    h = sc.home(run.pos, run.size, sc.table_log2(0, 600), True)
    assert sc.table_log2(0, 600) == 11 and np.bincount(h - h.min()).tolist() == [512, 88]
    # ending at size - 1: the last record is the home of the run's tail, and 2 entries per record send the chain on to record 0
    end = sc.dir_case("run-600-end")
    h = sc.home(end.pos, end.size, 11, True)
    assert int(end.pos[-1]) == end.size - 1 and h.max() == (1 << 11) - 1 and (h == h.max()).sum() == 511 > 2
    small = sc.dir_case("run-600-4099")
    h = sc.home(small.pos, small.size, 11, True)
    assert small.size == 4099 and len(small.pos) == 600 and sc.table_log2(0, 600) == 11
    per = np.bincount(h - h.min())
    assert per[0] == 3 and np.all(per[1:-1] == 2) and per[-1] == 1 and len(per) == 300         # one bit too many, 299 full records to pass
    assert sc.home([int(small.pos[0]) - 1], 4099, 11, True)[0] == h.min() - 1
    # the other layout scatters the same run: a record each
    h0 = sc.home(run.pos, run.size, 11, False)
    assert len(set(h0.tolist())) == 600


def test_home_matches_the_definition():
    for size in (4099, 1 << 20, (1 << 30) + 77):
        idx = np.array([0, 1, size // 2, size - 2, size - 1], dtype=np.uint64)
        for ordered in (True, False):
            mul = (2 ** 64 - 1) // size if ordered else 0x9E3779B97F4A7C15
            want = [((int(i) * mul) % 2 ** 64) >> (64 - 12) for i in idx]
            assert sc.home(idx, size, 12, ordered).tolist() == want
        assert sc.home(idx, size, 12, True).tolist() == sorted(sc.home(idx, size, 12, True).tolist())    # records in order of the slot


# ---- map cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sc.MAP_KS)
def test_map_case(k):
    c = sc.map_case(k)
    g = c.groups
    assert all(len(km) == k for name, rows in g.items() if not name.startswith("length") for km in rows)
    assert ("palindrome" in g) == (k % 2 == 0) and ("length-k-1" in g) == (k > 1) and ("length-k+1" in g) == (k < 128)
    for km in g.get("palindrome", []):
        assert sc.revcomp(km) == km
    for km, rc in zip(g["random"], g["revcomp"]):
        assert ocapi.canonical(km) == ocapi.canonical(rc) and (km != rc or k == 1)
    assert ocapi.canonical(b"A" * k) == ocapi.canonical(b"T" * k) == b"A" * k
    assert all(len(km) == k - 1 for km in g.get("length-k-1", [])) and all(len(km) == k + 1 for km in g.get("length-k+1", []))
    assert not any(sc.is_regular(km, k) for name in g if name.startswith(("length", "irregular")) for km in g[name])
    named = [i for i in (0, 31, 32, k - 1) if i < k]
    assert {n for n in g if n.startswith("differ-at-")} == {"differ-at-%s" % ("last" if i == k - 1 else i) for i in named}
    for i in named:
        tag = "last" if i == k - 1 else str(i)
        rows = g["differ-at-%s" % tag]
        per = len(rows) // 4
        for j in range(4):                                     # the variants of one anchored key differ at base i alone ...
            fam = rows[j * per:(j + 1) * per]
            assert len(set(fam)) == per >= 2
            for km in fam[1:]:
                assert [p for p in range(k) if km[p] != fam[0][p]] == [i]
            if k > 1:
                assert all(ocapi.canonical(km) == km for km in fam)      # ... and are stored as written
            if k <= sc.MAX_PACKED_K and k > 1:                 # ... so the named base differs in the L-form half it belongs to
                forms = [sc.lform(km) for km in fam]
                for lo, hi in forms[1:]:
                    dlo, dhi = lo ^ forms[0][0], hi ^ forms[0][1]
                    if i < 32:
                        assert dhi == 0 and dlo != 0 and dlo & ~(3 << (2 * i)) == 0
                    else:
                        assert dlo == 0 and dhi != 0 and dhi & ~(3 << (2 * (i - 32))) == 0
        for km in g["irregular-at-%s" % tag]:
            assert km[i] in sc.IUPAC and all(ch in b"ACGT" for p, ch in enumerate(km) if p != i)
    if k in (33, 63, 64):                                      # both sides of the split between the halves
        assert "differ-at-31" in g and ("differ-at-32" in g or k == 33) and 32 in named
    if k > sc.MAX_PACKED_K:
        assert not any(sc.is_regular(km, k) for km in c.rows)  # every key takes the host's list
    keys, rows = sc.stride_k_rows(k)
    assert rows.shape == (16, k) and not (rows == 0).any() and bytes(rows[3]) == keys[3]


def test_recorded_slot_kmers_hit_the_one_bit_block():
    kmers, h = sc.slot_kmers()
    assert len(kmers) == len(set(kmers)) == 24 and all(len(km) == sc.K and set(km) <= set(b"ACGT") for km in kmers)
    assert np.all(h % np.uint64(sc.SLOT_SIZE) == sc.SLOT) and sc.SLOT // sc.BLOCK_BITS == 256 and sc.SLOT == sc.SLOT_SIZE - 1
    first = sc.random_kmers(sc.SLOT_SEED, 200000, sc.K)        # the search's first batch, redone: the file's first k-mers come from it
    hit = [first[i] for i in np.flatnonzero(sc.hashes(first) % np.uint64(sc.SLOT_SIZE) == sc.SLOT)]
    assert hit == kmers[:len(hit)]


def test_lform_halves():
    km = b"C" + b"A" * 30 + b"G" + b"T" + b"A"
    assert sc.lform(km) == (1 | 2 << 62, 3)


def test_wrap_keys_start_at_the_last_record():
    keys, idx = sc.wrap_keys()
    assert len(keys) == len(set(keys)) >= 40 and set(idx.tolist()) == {sc.WRAP_SIZE - 1, sc.WRAP_SIZE - 2}
    assert min((idx == sc.WRAP_SIZE - 1).sum(), (idx == sc.WRAP_SIZE - 2).sum()) >= 20
    cap = sc.table_log2(len(keys), 0)
    assert cap == 10 and np.all(sc.home(idx, sc.WRAP_SIZE, cap, True) == (1 << cap) - 1)   # every chain runs past the last record
    assert np.array_equal(idx, sc.hashes(keys) % np.uint64(sc.WRAP_SIZE))


def test_growth_batches_grow_the_table_four_times():
    sizes, rows = [], 0
    for n in sc.GROWTH_BATCHES:
        rows += n
        sizes.append(sc.table_log2(rows, 0))
    assert sizes == [10, 13, 15, 17, 20]                       # created, then four rehashes


# ---- the oracle's map on the groups the device splits between its table and the host's list -------------------------------------
@pytest.mark.parametrize("k", [1, 33, 64, 65])
def test_oracle_map_counts_distinct_canonical_keys(k):
    c = sc.map_case(k)
    om = ocapi.KMAP()
    for km in c.rows:
        om.add_key(km)
    regular = {ocapi.canonical(km) for km in c.rows if sc.is_regular(km, k)}
    assert len(om) >= len(regular) and (k <= 64 or not regular)
    assert all(om.test_key(km) for km in c.rows)


# ---- sparse import ------------------------------------------------------------------------------------------------------------
def test_sparse_refusals_break_one_rule_in_one_place():
    clean = sc.sparse_clean()
    assert len(clean) == sc.SPARSE_N > 2 * sc.TPB and np.all(np.diff(clean.astype(np.int64)) > 0) and int(clean[-1]) < sc.SPARSE_SIZE
    assert len(sc.SPARSE_REFUSALS) == 8
    for name, make in sc.SPARSE_REFUSALS.items():
        p = make().astype(np.int64)
        bad = np.flatnonzero(np.diff(p) <= 0) + 1
        if name.startswith("size"):
            assert len(bad) == 0 and (p >= sc.SPARSE_SIZE).sum() == 1 and p[-1] == sc.SPARSE_SIZE
            assert len(p) - 1 == (256 if name.endswith("256") else sc.SPARSE_N - 1)
        else:
            kind, i, j = name.split("-")
            assert bad.tolist() == [int(j)] and int(j) == int(i) + 1 and p.max() < sc.SPARSE_SIZE
            assert (p[int(j)] == p[int(i)]) == (kind == "equal")
    # element 256 is the first thread of the second workgroup: its neighbour is read across the boundary
    assert {"equal-255-256", "descending-255-256"}.issubset(sc.SPARSE_REFUSALS)
