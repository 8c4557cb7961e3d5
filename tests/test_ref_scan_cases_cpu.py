"""tests/ref_scan_cases.py proved without a GPU: the restatement of the reference's window loop equals the oracle's mo_ref_scan on
every setup; every case meets the condition its expected result rests on -- one set bit of the context filter per claimed window,
the oracle's filter equal to the one made from the restated contexts -- and every seam a case names is where the case puts it.  A
case that cannot establish one of these fails here: nothing is skipped."""
import numpy as np
import pytest

import ref_scan_cases as rc
from oracle import capi as ocapi

IDS = rc.case_ids()
ACGT = set(b"ACGT")


def test_every_seam_is_named_by_a_case():
    table = {s: [n for n in IDS if s in rc.case(n).seams] for s in rc.SEAMS}
    assert all(table.values()), [s for s, v in table.items() if not v]
    named = {s for n in IDS for s in rc.case(n).seams}
    assert named <= set(rc.SEAMS), named - set(rc.SEAMS)
    for S in rc.SETUPS.values():                                # the full table on four setups, every other setup has the reduced one's seams
        mine = {s for n in IDS if rc.case(n).setup == S.name for s in rc.case(n).seams}
        assert {"err-at-off", "len-r", "w8-tail", "wg-256", "wg-2048", "bad-base"} <= mine, S.name
        assert ("quirk" in mine) == bool((S.ref_k - S.k) & 1) and (S.table != "full" or set(rc.SEAMS) - {"quirk", "no-quirk", "pal-kmer", "pal-context", "short", "err-below-off"} <= mine)
    assert [S.name for S in rc.SETUPS.values() if S.table == "full"] == ["35-43", "35-44", "63-64", "33-64"]
    assert {(S.k, S.ref_k) for S in rc.SETUPS.values()} == {(35, 43), (35, 63), (35, 44), (64, 64), (63, 64), (33, 64), (32, 33), (17, 18), (16, 17), (9, 9), (31, 42), (21, 29), (64, 65),
                                                            (100, 128)}
    bits = {S.bits for S in rc.SETUPS.values()}
    assert {1 << 27, 1000003, (1 << 33) + 12345} <= bits


@pytest.mark.parametrize("setup", [s for s in rc.SETUPS if rc.SETUPS[s].table != "giant"])
@pytest.mark.parametrize("which", ["even", "all", "thirds"])
def test_the_restatement_equals_the_oracle(setup, which):
    """`bf` from the restated centres of some windows, the oracle's scan, and the context filter made from the restated contexts of
    the same windows: equal, on a contig with an N and a lower-case g (and on contigs shorter than ref_k)"""
    S = rc.setup(setup)
    off = (S.ref_k - S.k) // 2
    for length in (S.ref_k + 2 * S.k + 150, S.ref_k - 1, off + 1, S.ref_k):
        if length <= off:
            continue
        contig = rc.rand(length, "restatement-" + setup, 0)
        if length > S.ref_k + 60:
            contig = rc.put(rc.put(contig, S.ref_k + 9, b"N"), S.ref_k + S.k + 30, b"g")
        ws = rc.windows(contig, S.k, S.ref_k)
        assert len(ws) == max(1, length - S.ref_k + 1)
        pick = [i for i in range(len(ws)) if which == "all" or (which == "even" and i % 2 == 0) or (which == "thirds" and i % 3 == 1)]
        obf = rc.oracle_bf(S, [ws[i][0] for i in pick])
        octx, mine = ocapi.BF(S.bits), ocapi.BF(S.bits)
        ocapi.ref_scan(obf, octx, contig, S.k, S.ref_k)
        for i in pick:
            mine.add_key(ws[i][1])
        if which == "all":                                      # whatever collides: every window hits, every context goes in
            assert np.array_equal(octx.words(), mine.words()), (setup, which, length)
        elif S.k >= 16 and S.bits > 1 << 26:                    # (no repeated k-mers and no collisions at this size: asserted, not assumed)
            assert octx.popcount() == len(pick)
            assert np.array_equal(octx.words(), mine.words()), (setup, which, length)
        else:                                                   # a small k or filter: an unpicked window may hit; the picked ones must all be there
            assert not (mine.words() & ~octx.words()).any()
    with pytest.raises(ValueError):
        rc.windows(b"A" * (off - 1), S.k, S.ref_k) if off else rc.windows(b"", S.k, S.ref_k + 2)


def test_the_quirk_windows_hold_a_gapped_string():
    """worked by hand for k = 3, ref_k = 6 (off = 1): window 0 tests bases 1..3; the append is reference[p - 1], one base ahead of
    a slide, so window 1 tests bases 2, 3, 5 and window 2 bases 3, 5, 6; from window k = 3 on the string is bases w + 2 .. w + 4"""
    ws = rc.windows(b"ACGTTGCAAT", 3, 6)
    assert [c for c, _ in ws] == [b"CGT", b"GTG", b"TGC", b"GCA", b"CAA"]
    assert [x for _, x in ws] == [b"ACGTTG", b"CGTTGC", b"GTTGCA", b"TTGCAA", b"TGCAAT"]
    assert [c for c, _ in rc.windows(b"ACGTTGCAAT", 2, 6)] == [b"GT", b"TT", b"TG", b"GC", b"CA"]      # even: the plain centred k-mer
    assert rc.windows(b"ACGT", 3, 6) == [(b"CGT", b"ACGT")] and rc.windows(b"AC", 3, 6) == [(b"C", b"AC")] and rc.windows(b"A", 3, 6) == [(b"", b"A")]


def test_the_recorded_seeds_are_what_the_search_finds():
    """for the setups whose search is cheap (the small filter, where collisions are likeliest, and k = 9); every other case's seed is
    held by the condition test below"""
    for name in ("31-42", "9-9"):
        found = rc.find_seeds({name})
        assert found == {n: s for n, s in rc.SEEDS.items() if n.startswith(name + "/")}
    assert all(n.replace("/nb-B", "/nb-A") in IDS and s > 0 for n, s in rc.SEEDS.items())


@pytest.mark.parametrize("setup", [S.name for S in rc.SETUPS.values() if S.table == "full"])
@pytest.mark.parametrize("P", [0, 1, 31])
def test_two_neighbours_scanned_into_one_filter_keep_one_bit_per_window(setup, P):
    """what the GPU file's two-call test expects: no window of A shares a bit with a window of B"""
    A, B = rc.case("%s/nb-A%d" % (setup, P)), rc.case("%s/nb-B%d" % (setup, P))
    S = rc.setup(setup)
    assert A.buffer == B.buffer == A.contig + B.contig and A.extra == B.extra
    obf = rc.oracle_bf(S, rc.bf_keys(A) + rc.bf_keys(B))
    octx = ocapi.BF(S.bits)
    ocapi.ref_scan(obf, octx, A.contig, S.k, S.ref_k)
    ocapi.ref_scan(obf, octx, B.contig, S.k, S.ref_k)
    assert octx.popcount() == len(A.hits) + len(B.hits)
    whole = ocapi.BF(S.bits)                                    # scanned as ONE contig the straddling windows hit as well: they are what must stay out
    ocapi.ref_scan(obf, whole, A.buffer, S.k, S.ref_k)
    assert len(np.setdiff1d(whole.set_positions(), octx.set_positions())) == S.ref_k - 1


@pytest.mark.parametrize("name", IDS)
def test_case_meets_the_condition_and_holds_what_it_says(name):
    c = rc.case(name)
    S = rc.setup(c.setup)
    k, r = S.k, S.ref_k
    d = r - k
    off, off_slide = d // 2, d - d // 2
    contig, cl = c.contig, c.claims
    assert len(contig) == c.length and c.offset + c.length <= len(c.buffer) and max(c.buffer, default=0) < 128
    assert len(c.buffer) <= 20000
    # the condition
    obf, octx = rc.expected(c)
    assert octx.popcount() == len(c.hits), (octx.popcount(), len(c.hits))
    assert np.array_equal(octx.set_positions(), rc.claimed_positions(c))
    assert 0 < obf.popcount() <= len(set(rc.bf_keys(c))) or not c.hits
    if c.err:
        assert c.length <= off and not c.hits and not c.extra
        if c.length < off:
            with pytest.raises(ValueError):
                rc.windows(contig, k, r)
        else:
            assert rc.windows(contig, k, r) == [(b"", contig)]
        return
    ws = rc.windows(contig, k, r)
    nw = len(ws)
    assert nw == rc.n_windows(c.length, r) and all(0 <= w < nw for w in c.hits) and len(set(c.hits)) == len(c.hits)
    if "n_windows" in cl:
        assert nw == cl["n_windows"]
    if "short" in c.seams:
        assert off < c.length < r and ws == [(contig[off:off + k], contig)] and len(ws[0][0]) == min(k, c.length - off) and len(c.hits) in (0, 1)
    if "w8-tail" in c.seams:
        assert 1 <= nw <= rc.REF_SCAN_W + 1 and len(c.hits) == nw
    if "wg-256" in c.seams:
        assert nw - rc.TPB in (-1, 0, 1)
    if "wg-2048" in c.seams:
        assert nw - rc.TPB * rc.REF_SCAN_W in (-1, 0, 1)
        assert c.hits == tuple(range(0, nw, 2)) if "even" in c.seams else {0, min(2047, nw - 1), nw - 1} <= set(c.hits)
    if cl.get("quirk"):                                         # the claimed quirk windows' strings are no k-mers of the contig
        assert d & 1 and nw > k + 1
        for w in c.hits:
            if w == 0:
                assert ws[w][0] == contig[off:off + k]
            elif w < k:
                assert ws[w][0] == contig[w + off:off + k] + contig[off_slide + k:w + off_slide + k]
                assert ws[w][0] not in (contig[w + off:w + off + k], contig[w + off_slide:w + off_slide + k])      # neither true slide gives it
            else:
                assert ws[w][0] == contig[w + off_slide:w + off_slide + k]
        assert set(c.hits) & set(range(1, k)) or c.hits in ((0,), (k,))
    if "no-quirk" in c.seams:
        assert not d & 1 and all(ws[w][0] == contig[w + off:w + off + k] for w in range(nw)) and c.hits == (0, 1, k - 1, k)
    if cl.get("pal_kmers"):
        assert k % 2 == 0 and all(ce == rc.revcomp(ce) for ce, _ in ws) and nw == (2 if r % 2 == 0 else 1) and len(c.hits) == nw
    if "pal_context" in cl:
        w = cl["pal_context"]
        assert ws[w][1] == rc.revcomp(ws[w][1]) and w in c.hits and r % 2 == 0
    bad = [i for i, ch in enumerate(contig) if ch not in ACGT]
    assert bad == sorted(cl.get("bad", []))
    if bad:
        dirty = [w for w in range(nw) if any(w <= q < w + r for q in bad)]
        assert dirty and len(dirty) < nw and set(dirty) <= set(c.hits) or "bad-run" in c.seams
        assert set(c.hits) - set(dirty)                         # clean windows are claimed too: both kernels must deliver
        for s in c.seams:
            if s.startswith("bad-bit-"):                        # thread 0's span starts at the contig's base 0: the base's number is its bit
                assert bad == [int(s[8:])] and bad[0] < rc.REF_SCAN_W + r - 1 + 64
    if name.endswith("/N-run"):
        run = r + 9
        assert contig[r + 3:r + 3 + run] == b"N" * run and run > r + 8
        inside = [w for w in range(nw) if ws[w][0] == b"N" * k]
        assert inside and set(c.hits) == set(range(nw)) - set(inside) and any(b"N" in ws[w][0] for w in c.hits)
    if name.endswith("/iupac-run"):
        assert len(bad) == r + 9 and bad == list(range(r + 3, 2 * r + 12)) and len(c.hits) == nw and any(set(ws[w][1]).isdisjoint(ACGT) for w in c.hits)
    if name.endswith("/N-two"):
        assert bad[1] - bad[0] == r and not any(q in bad for q in range(bad[0] + 1, bad[0] + 1 + r - 1)) and len(c.hits) == nw
    if "letter" in cl:
        w, where = cl["letter"]
        ch = contig[bad[0]] if bad else None
        spot = {"first": ws[w][1][0], "last": ws[w][1][-1], "centre": ws[w][0][k // 2]}[where]
        lower = [i for i, x in enumerate(contig) if x in b"acgt"]
        assert len(bad) == 1 and spot == ch and w >= k and w in c.hits and (lower == bad or not lower)
    for s in c.seams:
        if s.startswith("offset-"):
            assert c.offset % 32 == int(s[7:]) and ("o-zero" in c.seams) == (c.offset % 32 == 0)
    if "buffer-end" in c.seams:
        assert c.offset + c.length == len(c.buffer) and c.offset % 32
    if "neighbours" in c.seams:
        A_len = c.offset or c.length
        assert c.extra and set(c.extra) - {ws[w][0] for w in c.hits} and len(c.hits) == nw
        assert A_len % 32 == cl["neighbour"] and len(c.buffer) > A_len + r and c.offset in (0, A_len)
        AB = c.buffer
        assert all(AB[w + off_slide:w + off_slide + k] in c.extra for w in range(A_len - r + 1, A_len))    # every window that straddles A|B
        if c.offset:
            assert "B-starts-at-%d" % (c.offset % 32) in c.seams and (not d & 1 or nw > k)
