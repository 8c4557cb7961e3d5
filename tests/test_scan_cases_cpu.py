"""tests/scan_cases.py proved without a GPU: every seam is named by a case, every case's rows sit where the case says (the
oracle's hash, one k-mer at a time, and the restated arithmetic), every precondition a case's name states holds on the oracle
alone, the restated plan gives the form, layout and spill count each case claims, and the multiplicity identity that lets a
table of millions of rows cost the oracle a pool of thousands holds against a plain row-by-row oracle scan.  A case that cannot
establish one of these fails here: nothing is skipped."""
import time

import numpy as np
import pytest

import scan_cases as sc
from oracle import capi as ocapi

U = np.uint64
IDS = sc.case_ids()


@pytest.fixture(scope="module")
def built():
    """(case, oracle state after the scan, model) of every case, made once"""
    out = {}
    for name in IDS:
        c = sc.case(name)
        obf, octx, omap = sc.expected(c)
        out[name] = (c, obf, octx, omap, sc.model(c, obf.words()))
    return out


def test_every_seam_is_hit_by_a_case_that_names_it():
    table = {s: [n for n in IDS if s in sc.case(n).seams] for s in sc.SEAMS}
    assert all(table.values()), [s for s, v in table.items() if not v]
    named = {s for n in IDS for s in sc.case(n).seams}
    assert named <= set(sc.SEAMS), named - set(sc.SEAMS)
    assert all(sc.case(n).seams and sc.case(n).seam for n in IDS)
    assert {sc.case(n).family for n in IDS} == set("ABCDEFGH")


def test_every_pool_row_hashes_to_the_slot_the_pool_records():
    """EVERY row of every pool, one k-mer at a time, through another route than the pool's own (mo_canonical, then mo_xxh3_64, where
    the pool used mo_bf_hash): every selection by word, slice, sub-slice or bin is arithmetic on these slots.  A sample of each
    pool, and its found or constructed rows, through a third: a fresh oracle filter takes the centre k-mer (add_key) and its one
    set position is the slot"""
    for name in sorted({sc.case(n).setup for n in IDS}):
        s = sc.setup(name)
        again = np.array([ocapi.xxh3_64(ocapi.canonical(km)) % s.bits for km in s.centres], dtype=U)
        assert np.array_equal(again, s.slot), (name, np.flatnonzero(again != s.slot)[:5])
        rows = np.unique(np.concatenate([np.arange(0, len(s.rkmers), 97), np.arange(max(0, len(s.rkmers) - 80), len(s.rkmers))]))
        for i in rows:
            f = ocapi.BF(s.bits)
            f.add_key(s.centres[i])
            assert f.set_positions().tolist() == [int(s.slot[i])], (name, i)
            assert s.centres[i] == s.rkmers[i][s.off:s.off + s.k] and len(s.rkmers[i]) == s.ref_k
        assert (s.word[s.open] % 2 == 0).all() and (s.word[s.closed] % 2 == 1).all()
        assert np.array_equal(s.word, (s.slot // U(1 << (s.shift + 6))).astype(np.int64)) and s.word.max() < s.nwords
        hi, lo = s.hi[rows], s.lo[rows]                         # the packed rows spell the ref_k-mers (what the oracle's packed scan unpacks)
        for j, i in enumerate(rows):
            v = (int(hi[j]) << 64) | int(lo[j])
            assert bytes(b"ACGT"[(v >> (2 * (s.ref_k - 1 - q))) & 3] for q in range(s.ref_k)) == s.rkmers[i]


def test_found_slot_rows_sit_in_their_slots():
    G = sc.setup("slots")
    assert G.bits == 1 << 14 and (G.shift, G.nwords) == (6, 4)
    assert sc.SLOT_ROWS == sc.find_slot_rows()                  # the literals are what the recorded search finds
    assert sorted(sc.SLOT_ROWS) == sorted(sc.SLOT_TARGETS)
    for target in sc.SLOT_TARGETS:
        rows = G.slot_rows[target]
        assert len(rows) == 3 and G.kind[rows].tolist() == [0, 2, 3]
        assert len({G.centres[i] for i in rows}) == 3          # three k-mers that merely collide
        for i, literal in zip(rows, sc.SLOT_ROWS[target]):
            assert G.rkmers[i] == literal and ocapi.lib().mo_bf_hash(literal[4:39]) % G.bits == target
            f = ocapi.BF(G.bits)
            f.add_key(literal[4:39])
            assert f.set_positions().tolist() == [target]
    # what the targets are: the filter's ends, both sides of every gate word (4,096 slots), slice (2 words) and sub-slice (1 word)
    assert {0, G.bits - 1} <= set(sc.SLOT_TARGETS)
    for w in (1, 2, 3):
        assert {w * 4096 - 1, w * 4096} <= set(sc.SLOT_TARGETS)
    assert [t % 4096 // 64 for t in (4095, 4096)] == [63, 0]   # bit 63 of a gate word, bit 0 of the next


def test_the_recorded_counter_rows_are_what_the_search_finds():
    S = sc.setup("std")
    assert sc.H_PAIR == sc.find_h_pair(S) == S.h_pair
    hrow, hrow2, hmap = sc.H_PAIR
    for (which, count), rows in S.h.items():
        for row, src in zip(rows, (hrow, hrow2) if which == "bf" else (hmap,)):
            assert S.rkmers[row] == S.rkmers[src] and int(S.cnt[row]) == count and S.kind[row] == -2
    assert S.kind[hrow] in (0, 2) and S.kind[hrow2] in (0, 2) and S.kind[hmap] == 1


@pytest.mark.parametrize("name", ["A-carry-gated-left257", "B-allhit-e1-n257", "C-reset-subs-hits-first", "G-slots-direct-ord0", "G-palindrome-direct", "G-refscan-context",
                                  "G-palindrome-tickets", "C-reset-bins-hits-first", "H-copies-65536-w0-rc0-direct", "H-single-65536-w1-rc0-subs", "H-map-2^32-rc0-direct", "H-zero-and-max-w0-rc0-direct", "A-rows12-maxcount-r33"])
def test_multiplicity_identity_against_a_row_by_row_scan(name):
    c = sc.case(name)
    s = sc.setup(c.setup)
    obf, octx, omap = sc.expected(c)
    rbf, rctx, rmap = sc.oracle_index(c)
    hi, lo, cnt = sc.table(c)
    ocapi.kmc_scan_packed(rctx, rbf, rmap, hi, lo, cnt, s.k, s.ref_k)
    assert np.array_equal(obf.words(), rbf.words()) and np.array_equal(octx.words(), rctx.words())
    assert np.array_equal(obf.counts(), rbf.counts()) and dict(omap.items()) == dict(rmap.items())
    assert obf.counts().any() or any(v for _, v in omap.items())


def test_plan_arithmetic_pins():
    """numbers worked out by hand from ticket_layout / sub_layout / scan_plan"""
    sub = dict(gate_log2=20, use_sub=1, sub_min_log2=0, sub_words_log2=5)
    p = sc.plan(1 << 20, dict(sub, sub_grid=1), 3 * 16384, False)
    assert (p["form"], p["nbins"], p["nseg"], p["segcap"], p["parts"], p["bin_shift"]) == ("subs", 8, 1, 9280, 1, 17)   # (49152 / 8) * 1.5 + 64 -> 9280
    p = sc.plan(1 << 20, sub, 9 * 16384, False)
    assert (p["nseg"], p["parts"], p["ucap"]) == (9, 8, 2 * p["segcap"])
    p = sc.plan(1 << 22, dict(sub, sub_words_log2=1, sub_grid=4096), 1027 * 16384, False)
    assert (p["nbins"], p["nseg"], p["parts"], p["segcap"]) == (512, 1024, 1, 160)      # sub_grid beyond SB_MAXB is clamped to it
    tk = dict(gate_log2=30, pregate_log2=8, use_sub=0, ticket_min_log2=0)
    p = sc.plan(10 * 4096, tk, 5005, False)
    assert (p["form"], p["nbins"], p["nseg"], p["segcap"], p["bin_shift"]) == ("tickets", 5, 5, 688, 13)                # (2048 / 5) * 1.5 + 64 -> 688
    p = sc.plan(10 * 4096, dict(tk, scan_chunk_log2=10), 2051, True)
    assert (p["chunk"], sc.last_chunk(p, 2051)) == (1024, (2048, 3))
    assert sc.plan(1 << 20, dict(gate_log2=20), 1000, False)["form"] == "direct"
    assert sc.plan(1 << 20, dict(gate_log2=14, pregate_log2=10, use_partition=1, use_pregate=2), 1000, False)["nbins"] == 32
    assert sc.plan(1 << 20, dict(gate_log2=14, pregate_log2=10, use_partition=1, use_pregate=2), 1000, True)["form"] == "direct"
    assert sc.plan(1 << 20, dict(sub, use_summary=0), 1000, False)["form"] == "direct"
    assert sc.gate_geometry((1 << 18) + 77, 11) == (8, 1025, 17) and sc.gate_geometry(1 << 33, 14) == (19, 16384, 256)


@pytest.mark.parametrize("name", IDS)
def test_case_holds_what_it_says(built, name):
    c, obf, octx, omap, m = built[name]
    s = sc.setup(c.setup)
    order = c.order                                            # (made once: the largest are built on demand)
    cl, p, n = c.claims, m["plan"], len(order)
    slots = s.slot[order]
    opts = dict(c.opts)
    assert n >= 1 and order.min() >= 0 and order.max() < len(s.rkmers)
    assert m["form"] == cl["form"]
    assert m["n_open"][0] == m["n_open"][1], "the open rows of this case are not exact"
    for key in ("nbins", "spilled", "n_hits"):
        if key in cl:
            assert m[key] == cl[key], (key, m[key])
    for key in ("parts", "nseg"):
        if key in cl:
            assert p[key] == cl[key], (key, p[key])
    if c.entry.startswith("rows12"):
        assert 33 <= s.ref_k <= 44 and int(sc.counts_of(c)[order].max()) < 1 << (96 - 2 * s.ref_k)
    if "maxcount" in cl:
        assert cl["maxcount"] == (1 << (96 - 2 * s.ref_k)) - 1
    r0, nr = sc.last_chunk(p, n)
    if cl.get("all_hit"):                                       # every row's slot is a set bit, and no row is blocked
        assert sc.bits_set(obf.words(), slots).all() and m["n_hits"] == n and not any(octx.test_key(s.rkmers[i]) for i in set(order.tolist()))
    if cl.get("spilled_positive") and m["spilled"] is not None:
        assert m["spilled"] > 0
    if "exact_fill" in cl:
        b, want = cl["exact_fill"]
        f = sc.fills(p, slots[r0:])
        assert f[b].max() == f[b].sum() == want and (np.delete(f, b, axis=0) <= p["segcap"]).all()
        assert m["spilled"] == cl["spilled"] == max(0, want - p["segcap"])
        if "segcap" in name:
            assert abs(want - p["segcap"]) <= 1
    if "modes" in cl:
        assert sc.sub_tile_modes(p, slots[r0:]) == cl["modes"]
    if "left" in cl:                                            # a stage of exactly `left` rows is looked at by flush_if_above
        sure = np.isin(slots, s.slot[np.isin(s.kind, [0, 1, 2, 3])]) if opts.get("use_summary", 1) else np.ones(n, dtype=bool)
        trace = sc.direct_stage_trace(n, opts.get("scan_rows", 2), opts["scan_grid"], sure)
        assert any(cl["left"] in seen for seen in trace) and any(len(seen) > 1 for seen in trace), trace
        if cl["left"] == 256 and "gated-carry" in c.seams:     # ... kept, and the next iteration adds to it
            assert any(a == 256 and b > 256 for seen in trace for a, b in zip(seen, seen[1:]))
    if "probe-carry" in c.seams:
        assert opts["probe_grid"] == 1 and opts["hits_grid"] == 1 and m["n_open"] == (n, n)
    if name == "B-open0":
        assert m["n_open"] == (0, 0) and m["n_hits"] == 0
    if name == "B-hit0":
        assert obf.nset == 0 and m["n_open"] == (n, n) and sum(v for _, v in omap.items()) > 0
    if "chunk-counter-reset" in c.seams:
        first_hits = int(sc.bits_set(obf.words(), slots[:1024]).sum())
        assert p["chunk"] == 1024 and n == 2048 and {first_hits, m["n_hits"] - first_hits} == {0, 1024}
        assert m["n_open"][0] == (0 if first_hits else 1024)
    if c.family == "C":
        assert p["chunk"] == 1024 and n >= 1024
        if "chunks-bins" in c.seams or (p["form"] == "bins" and "chunk-counter-reset" in c.seams):
            assert p["nbins"] == 32 and p["nseg"] == 2 and not cl.get("spilled_positive")
    if c.family == "D" and p["form"] == "tickets":
        f = sc.fills(p, slots[r0:])
        grid = opts.get("ticket_gate_grid", 0) or max(8, sc.CUS // 8 * 8)
        walks = sc.ticket_walks(p, f, grid)
        assert sum(w[4] for w in walks) + m["spilled"] == nr    # every ticket is walked once, or spilled
        if "ticket-stage-full" in c.seams:                      # 16,384 passing tickets in one walk: four steps of 4,096, 512 per wave and step
            assert m["spilled"] == 0 and any(w[4] == 4 * sc.TKG_STEP for w in walks) and sc.TKG_WSTAGE - 512 == 3 * 512
        if cl.get("walks"):
            mine = [w for w in walks if w[0] == 0 and w[1] == 0]
            assert len(mine) >= 3 and all(w[3] == sc.TKG_SPW for w in mine[:3])
            seg = f[0, mine[1][2]:mine[1][2] + 64]
            assert (seg == 0).any() and (seg == sc.TK_TILE).any()
        if "ticket-second-tile" in c.seams:
            assert sc.ceil_div(nr, sc.TK_TILE) > p["nseg"] == 2048
        if "ticket-natural-overflow" in c.seams:
            assert "scan_bin_cap" not in opts and (f > p["segcap"]).any()
    if "sub-rest" in c.seams or "sub-one-step" in c.seams:
        assert (cl["exact_fill"][1] > sc.SBG_STEP) == ("sub-rest" in c.seams) and cl["exact_fill"][1] <= p["segcap"]
    if "sub-last-tile" in c.seams:
        assert n % sc.SB_TILE in (1, sc.SB_TILE - 1) and p["nseg"] == 1
        assert cl["last_row_hits"] and sc.bits_set(obf.words(), slots[-1:]).all() and not octx.test_key(s.rkmers[order[-1]])
    if "sub-partial-last" in c.seams:
        assert s.nwords % 8 == 7 and (s.word[order] == cl["last_word"]).any() and cl["last_word"] == s.nwords - 1
        assert np.isin(s.kind[order[s.word[order] == cl["last_word"]]], [0, 1, 2, 3]).any()
    if "sub-grid-clamp" in c.seams:
        assert opts["sub_grid"] > sc.SB_MAXB and sc.ceil_div(n, sc.SB_TILE) > sc.SB_MAXB == p["nseg"] and p["parts"] == 1 and m["spilled"] == 0
        f = sc.fills(p, slots)
        assert len({int(f[b, 0]) for b in range(8)} | {int(f[b, 1]) for b in range(8)}) > 1      # fills differ: a wrong lane's fill is a wrong count
    if "bin-second-iteration" in c.seams:
        assert sc.ceil_div(n, 1024) > p["nseg"] == 2048 and opts["scan_bin_rows"] == 4
    if "bin-one-bin" in c.seams:
        assert len(set((slots[np.isin(s.kind[order], [0, 1, 2, 3])] >> U(p["bin_shift"])).tolist())) == 1
    if c.family == "F":
        assert p["form"] == "bins" and (not opts.get("scan_bin_ring") or opts["scan_bin_ring"] * p["nbins"] <= 2048)
    if "context-twins" in c.seams:
        G = s
        for t, target in zip(G.twins, sc.SLOT_TARGETS):
            o = G.slot_rows[target][2]
            assert G.centres[t] == G.centres[o] and G.rkmers[t] != G.rkmers[o] and octx.test_key(G.rkmers[o]) and not octx.test_key(G.rkmers[t])
            assert obf.get_count(G.centres[t]) > 0              # the twin's count arrived, its blocked original's did not (the identity test compares the sums)
        strands = [G.rkmers[i] < sc.revcomp(G.rkmers[i]) for i in order]
        assert any(strands) and not all(strands)                # rows given as either strand of their canonical ref_k-mer
    if "key-and-bit" in c.seams:
        both = [i for i in set(order.tolist()) if s.kind[i] == 2]
        assert both and all(omap.test_key(s.centres[i]) and obf.test_key(s.centres[i]) for i in both)
    if "shared-record" in c.seams:
        bf, mp, _ = s.index_lists(c.indexed)
        rec = sc.map_records(s.bits, len(mp), obf.nset, [8193, 8194, 8195])
        assert len(set(rec)) == 1 and opts["map_ordered"] == 1 and sc.bits_set(obf.words(), np.array([8193, 8194, 8195], dtype=U)).all()
    if "palindrome" in c.seams:
        pal = [i for i in s.pal if s.centres[i] == sc.revcomp(s.centres[i])]
        assert s.k % 2 == 0 and len(pal) == len(s.pal) == 40 and np.isin(s.pal, order).all()
        assert any(obf.get_count(s.centres[i]) for i in pal) and any(omap.get_count(s.centres[i]) for i in pal)
    if "refscan-context" in c.seams:
        blocked = [i for i in set(order.tolist()) if s.kind[i] == 3]
        assert sc.index_of(c)[2] == [] and octx.nset >= len(blocked) > 100 and all(octx.test_key(s.rkmers[i]) for i in blocked)
    if "counter" in cl:
        for which, row, want in cl["counter"]:
            got = obf.get_count(s.centres[row]) if which == "bf" else omap.get_count(s.centres[row])
            assert got == want, (which, row, got, want)
            assert not octx.test_key(s.rkmers[row])
        if "contention" in c.seams:
            assert np.bincount(order).max() == 100000
        if cl["counter"][0][0] == "bf":                         # the two rows' bits are the two entries of one record, and nothing walks into it;
            rows = [r for _, r, _ in cl["counter"]]            # one is taken through 2^16 (or to its brink), the other is held at 7
            assert opts["map_ordered"] == 1 and len(rows) == 2 and cl["counter"][1][2] == 7 and cl["counter"][0][2] in (65535, 0, 1, 65534)
            bf, mp, _ = s.index_lists(c.indexed)
            pos = obf.set_positions()
            rec = sc.map_records(s.bits, len(mp), obf.nset, pos)
            mine = {rec[int(np.searchsorted(pos, s.slot[row]))] for row in rows}
            assert len(mine) == 1 and s.slot[rows[0]] != s.slot[rows[1]] and rec.count(min(mine)) == 2 and rec.count(min(mine) - 1) <= 2
    if cl.get("large"):
        assert n > 1 << 20


def test_the_large_cases_cost_the_oracle_their_pool():
    large = [n for n in IDS if sc.case(n).claims.get("large")]
    assert len(large) >= 5
    for name in large:
        c = sc.case(name)
        t0 = time.perf_counter()
        obf, octx, omap = sc.expected(c)
        dt = time.perf_counter() - t0
        assert dt < 1.0, (name, dt)
        assert obf.counts().any()
