"""The stores on the device against the oracle on the directed cases of tests/store_cases.py: the rank directory at every tile
and chunk seam of mg_bf_finalize, its scan by itself (mg_debug_tile_scan), the 64-bit total at the 2^32 limit, the directory
inside the records as the call-time lookups read it (mg_debug_bucket_count), the exact map at every k around the split of its
packed key, its batches and growths, and what sparse import refuses.  Everything is exact.  tests/test_store_cases_cpu.py
asserts, without a GPU, that each case holds what its name says and that the numpy model used at 2^32 agrees with the oracle."""
import numpy as np
import pytest

import store_cases as sc
from malva_amd import BF_ALT, BF_CTX, Context, MalvaError, synth
from malva_amd.capi import rows_of
from oracle import capi as ocapi

pytestmark = pytest.mark.gpu

MG_ERR_ARG, MG_ERR_STATE, MG_ERR_LIMIT = -1, -3, -5
WHICH = [BF_ALT, BF_CTX]
WHICH_IDS = ["alt", "ctx"]


@pytest.fixture(scope="module")
def ctx_of():
    """one context per filter size, shared by that size's cases: every case imports over what the last one left"""
    made = {}

    def get(size):
        if size not in made:
            made[size] = Context(sc.K, 43, size)
        return made[size]
    yield get
    for c in made.values():
        c.close()


def _oracle_counts(obf, kmers):
    return np.array([obf.get_count(km) for km in kmers], dtype=np.uint16)


def _state(ctx, which, c, obf, rows, dense):
    """everything the filter answers, against the oracle holding the same words and counters"""
    assert ctx.bf_info(which) == (c.size, len(c.pos), 1)
    mode, size, pos, counts = ctx.bf_export_sparse(which)
    assert (mode, size) == (1, c.size) and np.array_equal(pos, c.pos) and np.array_equal(counts, obf.counts())
    if dense:
        mode, size, words, counts = ctx.bf_export(which)
        assert (mode, size) == (1, c.size) and np.array_equal(words, obf.words()) and np.array_equal(counts, obf.counts())
    got, want = ctx.bf_get_count(which, rows), _oracle_counts(obf, c.probe)
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:5], got[got != want][:5], want[got != want][:5])


# ---- filter: import, rank directory, counters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH, ids=WHICH_IDS)
@pytest.mark.parametrize("name", sc.filter_case_ids())
def test_filter_case(ctx_of, name, which):
    c = sc.filter_case(name)
    ctx = ctx_of(c.size)
    obf = sc.oracle_filter(c.size, c.pos, c.counts)
    rows = rows_of(c.probe)
    if c.size <= 1 << 20:                                      # the dense words give the same state as the positions
        ctx.bf_import(which, 1, c.size, sc.words_of(c.size, c.pos), c.counts)
        _state(ctx, which, c, obf, rows, True)
    ctx.bf_import_sparse(which, 1, c.size, c.pos, c.counts)
    _state(ctx, which, c, obf, rows, True)
    for km, n in zip(c.probe, c.inc):                          # k-mers that meet at a slot, sums that wrap 65,536
        obf.increment(km, int(n))
    ctx.bf_increment(which, rows, c.inc)
    _state(ctx, which, c, obf, rows, False)


@pytest.mark.parametrize("which", WHICH, ids=WHICH_IDS)
@pytest.mark.parametrize("size", sc.TILE_SIZES)
def test_insert_route_and_a_second_finalize(size, which):
    kmers = sc.pool()[0][:6000]
    probe = sc.pool()[0][5000:7000]
    obf = ocapi.BF(size)
    for km in kmers:
        obf.add_key(km)
    obf.switch_mode()
    inc = np.random.default_rng(size % 991).integers(1, 70000, size=len(probe)).astype(np.uint32)
    with Context(sc.K, 43, size) as ctx:
        ctx.bf_insert(which, rows_of(kmers))
        for again in range(2):                                 # the second finalize rebuilds the directory over the same bits; counters restart
            ctx.bf_finalize(which)
            if again:
                obf.switch_mode()
            assert ctx.bf_info(which) == (size, obf.nset, 1)
            mode, _, words, counts = ctx.bf_export(which)
            assert mode == 1 and np.array_equal(words, obf.words()) and not counts.any()
            assert np.array_equal(ctx.bf_export_sparse(which)[2], obf.set_positions())
            for km, n in zip(probe, inc):
                obf.increment(km, int(n))
            ctx.bf_increment(which, rows_of(probe), inc)
            assert np.array_equal(ctx.bf_get_count(which, rows_of(probe)), _oracle_counts(obf, probe))
            assert np.array_equal(ctx.bf_export(which)[3], obf.counts())


# ---- the 64-bit total at the 2^32 limit ---------------------------------------------------------------------------------------
def test_total_of_2_to_32_set_bits_is_refused_and_two_fewer_accepted():
    size = 1 << 32
    words = np.full(size // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    kmers = sc.pool()[0][:400] + sc.pool()[0][:40]
    idx = sc.pool()[1][:400] % np.uint64(size)
    idx = np.concatenate([idx, idx[:40]])
    inc = np.random.default_rng(32).integers(1, 70000, size=len(kmers)).astype(np.uint32)
    with Context(sc.K, 43, size) as ctx:
        with pytest.raises(MalvaError) as e:                   # a total that wrapped at 32 bits would read 0 here and be accepted
            ctx.bf_import(BF_CTX, 1, size, words, np.zeros(0, np.uint16))
        assert e.value.code == MG_ERR_LIMIT
        assert ctx.bf_info(BF_CTX)[2] == 0                     # not finalised, and still usable:
        words[0] &= np.uint64(0xFFFFFFFFFFFFFFFE)
        words[-1] &= np.uint64(0x7FFFFFFFFFFFFFFF)
        ctx.bf_import(BF_CTX, 0, size, words, np.zeros(0, np.uint16))
        ctx.bf_finalize(BF_CTX)
        assert ctx.bf_info(BF_CTX) == (size, 4294967294, 1)
        # the model: every slot but 0 and 2^32 - 1 is set, rank = slot - 1, so k-mers share a counter exactly when they share a slot
        hit = (idx != 0) & (idx != np.uint64(size - 1))
        assert hit.sum() >= 400
        want = {}
        for i, n, h in zip(idx.tolist(), inc.tolist(), hit.tolist()):
            if h:
                want[i] = (want.get(i, 0) + n) & 0xFFFF
        assert not ctx.bf_get_count(BF_CTX, rows_of(kmers)).any()
        ctx.bf_increment(BF_CTX, rows_of(kmers), inc)
        got = ctx.bf_get_count(BF_CTX, rows_of(kmers))
        assert np.array_equal(got, np.array([want.get(i, 0) for i in idx.tolist()], dtype=np.uint16))


# ---- the tile scan by itself ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_ctx():
    c = Context(sc.K, 43, 1 << 16)
    yield c
    c.close()


def _scan_check(ctx, name):
    x = sc.scan_values(name)
    pre, total = sc.scan_model(x)
    got, got_total = ctx.tile_scan(x)
    assert got_total == total, (got_total, total)              # always, beyond 2^32 too
    # every prefix as the kernel stores it, modulo 2^32: those whose true value is below 2^32 are the true values
    bad = np.flatnonzero(got != (pre & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert bad.size == 0, (bad[:5], got[bad[:5]], pre[bad[:5]])


@pytest.mark.parametrize("name", sc.scan_case_ids())
def test_tile_scan(scan_ctx, name):
    """in the table's order on one context: the chunk totals' scratch is reused and resized between sizes"""
    _scan_check(scan_ctx, name)


def test_tile_scan_small_after_large_and_back(scan_ctx):
    for name in ("random-%d" % sc.SCAN_NS[-1], "ones-1", "random-8193", "ones-0", sc.BIG_SCAN, "random-16384", "ones-%d" % sc.SCAN_NS[-1]):
        _scan_check(scan_ctx, name)


# ---- the directory inside the records -------------------------------------------------------------------------------------------
def _dir_check(ctx, c, model, live):
    """every slot of the filter: the set ones give their rank and counter; all others -- the neighbours of set bits, the slots that
    share a home record with one under either layout, and the rest -- give (-1, 0)"""
    assert ctx.get_option("record_counters_live") == live
    rank, count = ctx.bucket_count(np.arange(c.size, dtype=np.uint64))
    want_rank = np.full(c.size, -1, dtype=np.int64)
    want_rank[model.pos.astype(np.int64)] = np.arange(len(model.pos))
    want_count = np.zeros(c.size, dtype=np.uint32)
    want_count[model.pos.astype(np.int64)] = model.counts
    bad = np.flatnonzero(rank != want_rank)
    assert bad.size == 0, (bad[:5], rank[bad[:5]], want_rank[bad[:5]])
    bad = np.flatnonzero(count != want_count)
    assert bad.size == 0, (bad[:5], count[bad[:5]], want_count[bad[:5]])


@pytest.mark.parametrize("copies", [0, 2], ids=["vectors", "record-copies"])
@pytest.mark.parametrize("ordered", [1, 0], ids=["ordered", "scattered"])
@pytest.mark.parametrize("name", sc.DIR_CASES)
def test_directory_case(name, ordered, copies):
    c = sc.dir_case(name)
    model = sc.FilterModel(c.pos, c.counts)
    hi, lo = synth.pack_ascii(synth.BASES[np.random.default_rng(1).integers(0, 4, size=(1000, 43))])
    with Context(sc.K, 43, c.size) as ctx:
        ctx.set_option("map_ordered", ordered)
        ctx.set_option("use_record_counters", copies)

        def check():
            _dir_check(ctx, c, model, 0)                       # nothing but a scan makes the records' copies current
            if copies:
                ctx.kmc_scan(hi, lo, np.zeros(1000, dtype=np.uint32))      # (adds nothing; publishes the counters into the records)
                _dir_check(ctx, c, model, 1)
                assert np.array_equal(ctx.bf_export(BF_ALT)[3], model.counts)

        with pytest.raises(MalvaError) as e:
            ctx.bucket_count(np.zeros(1, np.uint64))
        assert e.value.code == MG_ERR_STATE                    # no directory before the filter is finalised
        if c.keys_before:
            ctx.map_insert(rows_of(c.keys_before))
        ctx.bf_finalize(BF_CTX)
        ctx.bf_import_sparse(BF_ALT, 1, c.size, c.pos, c.counts)
        with pytest.raises(MalvaError) as e:
            ctx.bucket_count(np.array([0, c.size], np.uint64))
        assert e.value.code == MG_ERR_ARG
        check()
        ctx.bf_increment(BF_ALT, rows_of(c.probe), c.inc)
        model.increment(c.probe_idx, c.inc)
        check()
        ctx.map_insert(rows_of(c.keys_after))                  # the table grows: the directory is written again into the new records
        check()
        assert ctx.map_size() == len(c.keys_before) + len(c.keys_after)
        assert np.array_equal(ctx.bf_get_count(BF_ALT, rows_of(c.probe)), model.get_count(c.probe_idx))


# ---- the exact map --------------------------------------------------------------------------------------------------------------
def _absent(k):
    return sc.random_kmers(900 + k, 20, k)


def _map_check(ctx, om, probe):
    assert ctx.map_size() == len(om)
    rows = rows_of(probe)
    assert np.array_equal(ctx.map_test(rows), np.array([om.test_key(p) for p in probe]))
    got, want = ctx.map_get_count(rows), np.array([om.get_count(p) for p in probe], dtype=np.int32)
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:5], got[got != want][:5], want[got != want][:5])
    gk, gv = ctx.map_export()
    assert len(gk) == len(set(gk)) and dict(zip(gk, (int(v) for v in gv))) == dict(om.items())


def _insert(ctx, om, keys):
    for km in keys:
        om.add_key(km)
    ctx.map_insert(rows_of(keys))


def _increment(ctx, om, keys, seed):
    cnt = np.random.default_rng(seed).integers(1, 1 << 30, size=len(keys)).astype(np.int32)
    for km, n in zip(keys, cnt):
        om.increment(km, int(n))
    ctx.map_increment(rows_of(keys), cnt)


@pytest.mark.parametrize("k", sc.MAP_KS)
def test_map_case(k):
    c = sc.map_case(k)
    probe = c.rows + _absent(k)
    om = ocapi.KMAP()
    with Context(k, k, 1 << 16) as ctx:
        _insert(ctx, om, c.rows)                               # one batch: reverse complements, all-A / all-T and palindromes meet inside it
        _map_check(ctx, om, probe)
        # Regular keys (canonical form k long, pure ACGT, k <= 64) took the device table and the others the host's list:
        # mg_map_export writes the table's keys first and the host's list behind them, so the first rows of the export are
        # exactly the regular keys and the rest exactly the others.  (A pack_regular that sent a regular key to the host would
        # still answer every lookup; the scan, which reads the table alone, would never see the key.)
        canon = {sc.canonical_key(km) for km in c.rows}
        regular = {key for key in canon if sc.is_regular(key, k)}
        assert canon == {key for key, _ in om.items()} and (len(regular) >= 80 if 31 <= k <= 64 else k == 1 or not regular)
        gk, _ = ctx.map_export()
        assert set(gk[:len(regular)]) == regular and set(gk[len(regular):]) == canon - regular
        assert ctx.map_size() - len(canon - regular) == len(regular)
        _increment(ctx, om, probe + c.rows[::3], k)
        _map_check(ctx, om, probe)
        _insert(ctx, om, c.rows[::2])                          # met again from an earlier batch: back to 0 (kmap.hpp:111)
        _map_check(ctx, om, probe)
        # rows that fill their stride, no terminator
        keys, rows = sc.stride_k_rows(k)
        if k < 2:
            with pytest.raises(MalvaError) as e:
                ctx.map_insert(rows)
            assert e.value.code == MG_ERR_ARG
        else:
            for km in keys:
                om.add_key(km)
            ctx.map_insert(rows)
            assert ctx.map_test(rows).all()
            _map_check(ctx, om, probe + keys)


def test_map_batches_reset_only_what_an_earlier_batch_held():
    x, y, z, w = sc.random_kmers(77, 4, sc.K)
    om = ocapi.KMAP()
    with Context(sc.K, sc.K, 1 << 16) as ctx:
        _insert(ctx, om, [x, y, x])                            # the same key twice in one batch
        _increment(ctx, om, [x, y, sc.revcomp(x)], 1)
        _map_check(ctx, om, [x, y, z, w])
        _insert(ctx, om, [z, sc.revcomp(z), z])                # a new key, first row of its batch, three times
        _increment(ctx, om, [z, w], 2)
        _map_check(ctx, om, [x, y, z, w])
        _insert(ctx, om, [x])                                  # across two batches, after it was incremented: 0
        _map_check(ctx, om, [x, y, z, w])
        _increment(ctx, om, [x, y, z], 3)
        _insert(ctx, om, [w, y, sc.revcomp(y), z])             # across two batches and twice in the second
        _map_check(ctx, om, [x, y, z, w])
        assert om.get_count(y) == 0 and om.get_count(z) == 0 and om.get_count(x) != 0


@pytest.mark.parametrize("n", [255, 256, 257])
def test_map_batch_sizes(n):
    keys = sc.random_kmers(n, n, sc.K)
    om = ocapi.KMAP()
    with Context(sc.K, sc.K, 1 << 16) as ctx:
        _insert(ctx, om, keys)
        _increment(ctx, om, keys, n)
        _map_check(ctx, om, keys + _absent(sc.K))
        _insert(ctx, om, keys[-2:] + keys[:1])
        _map_check(ctx, om, keys + _absent(sc.K))


def test_map_four_growths_keep_ids_and_values():
    """five batches: the table as created (2^10), then 2^13, 2^15, 2^17 and 2^20 records -- four rehashes"""
    om = ocapi.KMAP()
    have = []
    with Context(sc.K, sc.K, 1 << 16) as ctx:
        for b, n in enumerate(sc.GROWTH_BATCHES):
            keys = sc.random_kmers(500 + b, n, sc.K)
            _insert(ctx, om, keys)
            have += keys
            _increment(ctx, om, have[::3], b)                  # counters set in between: ids and values must survive each rehash
            probe = have[::11] + keys[:50] + _absent(sc.K)
            assert np.array_equal(ctx.map_get_count(rows_of(probe)), np.array([om.get_count(p) for p in probe], dtype=np.int32))
            assert ctx.map_test(rows_of(probe[:-20])).all() and not ctx.map_test(rows_of(probe[-20:])).any()
        _map_check(ctx, om, have[::5] + _absent(sc.K))


@pytest.mark.parametrize("ordered", [1, 0], ids=["ordered", "scattered"])
def test_map_chain_past_the_last_record(ordered):
    keys, _ = sc.wrap_keys()
    om = ocapi.KMAP()
    with Context(sc.K, sc.K, sc.WRAP_SIZE) as ctx:
        ctx.set_option("map_ordered", ordered)
        _insert(ctx, om, keys)
        _increment(ctx, om, keys + keys[::2], 9)
        _map_check(ctx, om, keys + _absent(sc.K))
        ctx.bf_import_sparse(BF_ALT, 1, sc.WRAP_SIZE, np.array([sc.WRAP_SIZE - 2, sc.WRAP_SIZE - 1], np.uint64), np.array([7, 9], np.uint16))
        rank, count = ctx.bucket_count(np.arange(sc.WRAP_SIZE, dtype=np.uint64))     # the directory shares those records
        assert rank[-2:].tolist() == [0, 1] and count[-2:].tolist() == [7, 9] and (rank[:-2] == -1).all() and not count[:-2].any()
        _map_check(ctx, om, keys + _absent(sc.K))


@pytest.mark.parametrize("k", [33, 64])
def test_map_import_of_an_export_that_repeats_and_renames(k):
    c = sc.map_case(k)
    om = ocapi.KMAP()
    with Context(k, k, 1 << 16) as a, Context(k, k, 1 << 16) as b:
        _insert(a, om, c.rows)
        _increment(a, om, c.rows, k)
        keys, vals = a.map_export()                            # (compared with the oracle key by key in test_map_case)
        assert dict(zip(keys, (int(v) for v in vals))) == dict(om.items())
        present = c.groups["random"][:5]
        b.map_insert(rows_of(present))                         # already there when the file arrives
        b.map_increment(rows_of(present), np.full(5, 99, np.int32))
        ob = ocapi.KMAP()
        for km in present:
            ob.add_key(km)
            ob.increment(km, 99)
        # The file names every key, and the first of them again at the end with another value: the last row that names a key
        # gives its value, as when the reference reads the file row by row.  (That also settles the keys made from rows that
        # began with a lower-case letter: such a key is the text of a reverse complement, read again it is filed under the
        # other strand's text, and two rows of this file then name one key with two values.)
        assert any(sc.canonical_key(km) != km for km in keys)
        file_keys, file_vals = list(keys) + [keys[0]], np.concatenate([vals, vals[:1] + np.int32(7)])
        _replay(ob, file_keys, file_vals)
        b.map_import(file_keys, file_vals)
        bk, bv = b.map_export()
        assert dict(zip(bk, (int(v) for v in bv))) == dict(ob.items())
        probe = c.rows + _absent(k)
        assert np.array_equal(b.map_get_count(rows_of(probe)), np.array([ob.get_count(p) for p in probe], dtype=np.int32))


def _replay(ob, keys, vals):
    for km, v in zip(keys, vals):
        ob.add_key(km)
        ob.increment(km, int(v))


@pytest.mark.parametrize("n", [257, 3000])
def test_map_import_takes_the_last_row_that_names_a_key(n):
    """n rows over 40 keys in both orientations and 6 keys of the host's list, every row with a value of its own: rows of one
    key sit in different workgroups, and the last of them decides -- for new keys and for keys that were there before"""
    regular = sc.random_kmers(61, 40, sc.K)
    texts = regular + [sc.revcomp(km) for km in regular] + sc.map_case(sc.K).groups["irregular-at-32"] + sc.map_case(sc.K).groups["length-k+1"][:2]
    rng = np.random.default_rng(n)
    rows = [texts[i] for i in rng.integers(0, len(texts), size=n)]
    vals = rng.integers(-(1 << 31), 1 << 31, size=n).astype(np.int32)
    ob = ocapi.KMAP()
    with Context(sc.K, sc.K, 1 << 16) as ctx:
        _insert(ctx, ob, regular[:10] + texts[-3:])
        _increment(ctx, ob, regular[:10] + texts[-3:], 5)
        _replay(ob, rows, vals)
        ctx.map_import(rows, vals)
        _map_check(ctx, ob, texts + _absent(sc.K))
        again = rng.permutation(n)                             # the same rows in another order: other last rows
        _replay(ob, [rows[i] for i in again], vals[again])
        ctx.map_import([rows[i] for i in again], vals[again])
        _map_check(ctx, ob, texts + _absent(sc.K))


# ---- sparse import: what it refuses -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH, ids=WHICH_IDS)
@pytest.mark.parametrize("name", list(sc.SPARSE_REFUSALS))
def test_sparse_import_refuses_and_the_context_goes_on(name, which):
    bad = sc.SPARSE_REFUSALS[name]()
    clean = sc.sparse_clean()
    c = sc.filter_case("4099-full")
    with Context(sc.K, 43, sc.SPARSE_SIZE) as ctx:
        for mode in (0, 1):                                    # (mode 1 would also trip over popcount != n: mode 0 leaves the check to the kernel)
            with pytest.raises(MalvaError) as e:
                ctx.bf_import_sparse(which, mode, sc.SPARSE_SIZE, bad, sc.counts_of(len(bad)))
            assert e.value.code == MG_ERR_ARG and "strictly ascending" in str(e.value)
        ctx.bf_import_sparse(which, 1, sc.SPARSE_SIZE, clean, sc.counts_of(len(clean)))
        obf = sc.oracle_filter(sc.SPARSE_SIZE, clean, sc.counts_of(len(clean)))
        assert ctx.bf_info(which) == (sc.SPARSE_SIZE, len(clean), 1)
        mode, _, words, counts = ctx.bf_export(which)
        assert np.array_equal(words, obf.words()) and np.array_equal(counts, obf.counts())
        ctx.bf_finalize(which)                                 # and it still finalizes
        obf.switch_mode()
        for km, n in zip(c.probe, c.inc):
            obf.increment(km, int(n))
        ctx.bf_increment(which, rows_of(c.probe), c.inc)
        assert np.array_equal(ctx.bf_get_count(which, rows_of(c.probe)), _oracle_counts(obf, c.probe))
        assert np.array_equal(ctx.bf_export_sparse(which)[2], clean)
