"""The case table of tests/row_cases.py, proved without a GPU: every case holds every seam it claims, by the restated geometry and the
item spans alone; every seam of the list is claimed for every encoder it applies to; the item spans spell the bytes the plain formatters
of the existing test files make, and the second formatter of those files agrees where it has the case's fields; the geometry agrees
with a second statement made byte by byte; and each deliberate fault of a seam family changes, in the restatement, bytes of the case
that claims the seam (the faults that only misformat are also run on the device, by hand: see DESIGN.md)."""
import itertools
import math

import numpy as np
import pytest

import row_cases as rc

CASES = rc.cases()
BY_NAME = {c.name: c for c in CASES}
case_param = pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)


@case_param
def test_every_claimed_seam_is_hit(case):
    assert case.seams and len(set(case.seams)) == len(case.seams)
    assert 0 <= case.shift < 16 and all(0 <= cap < case.total() for cap in case.caps)
    for seam in case.seams:
        assert seam in rc.REQUIRED[case.encoder], "%s is not a seam of %s" % (seam, case.encoder)
        assert rc.holds(case, seam), "%s does not hold %s" % (case.name, seam)


def test_every_seam_is_claimed_for_every_encoder_it_applies_to():
    for enc, seams in rc.REQUIRED.items():
        assert len(set(seams)) == len(seams)
        claimed = {s: [c.name for c in CASES if c.encoder == enc and s in c.seams] for s in seams}
        for s in seams:
            print("%-5s %-32s %s" % (enc, s, ", ".join(claimed[s])))
        assert not [s for s in seams if not claimed[s]], enc
    print({enc: sum(c.encoder == enc for c in CASES) for enc in rc.REQUIRED})


def test_what_applies_where():
    """the window and capacity seams are the driver's and apply to all three; a value's split to the encoder that has the value"""
    text, bcf, info = (set(rc.REQUIRED[e]) for e in ("text", "bcf", "info"))
    driver = {s for s in info if not s.startswith("pow10")}
    assert driver < text and driver < bcf and info - driver == {"pow10-ac", "pow10-ns", "pow10-an"}
    assert {"int-split-10-pl", "gp-split-0-one", "gp-split-8-frac", "scan-n-16385", "pow10-gt2"} <= text - bcf
    assert {"bcf-split-4@3-gp", "gp-window-at-T100+0-dip", "gp-window-at-T1-1-hap", "desc-32768-pl", "desc-127-covs"} <= bcf - text
    assert len(text) == 114 and len(bcf) == 100 and len(info) == 40


@case_param
def test_the_formatters_agree(case):
    want, want_off = case.expected()
    assert np.array_equal(want_off, case.row_off())
    assert len(want) == case.total()
    assert case.joined() == want, "the item spans do not spell what the plain formatter makes"
    second = case.second()
    if second is not None:
        assert second[0] == want and np.array_equal(second[1], want_off), "the two formatters of the existing tests disagree"
    spans = case.spans()
    assert spans[0][4] == 0 and spans[-1][5] == case.total() and all(a[5] == b[4] for a, b in zip(spans, spans[1:]))


def test_the_second_formatter_sees_cases_of_both_encoders():
    seen = {c.encoder for c in CASES if c.second() is not None}
    assert seen == {"text", "bcf"}                                                # (the site tags have one restatement: info_text)


@case_param
def test_geometry_against_the_byte_by_byte_statement(case):
    off, total = case.row_off(), case.total()
    for cap in [total, total + 100] + list(case.caps) + [0, 1, total - 1, total // 2]:
        tiles = rc.geometry(off, case.shift, cap)
        size = min(total, cap)
        kind, win, outside = rc.store_map(tiles, size)
        want_kind, want_win = rc.store_map_brute(off, case.shift, cap)
        assert outside == 0, "a store outside the bytes in front of the capacity"
        assert np.array_equal(kind, want_kind) and np.array_equal(win, want_win), cap
        for t in tiles:
            assert [w.w0 for w in t.windows[1:]] == [w.w1 for w in t.windows[:-1]]
            for w in t.windows:
                assert 0 < w.w1 - w.w0 <= rc.FMT_WINDOW - w.mis and (case.shift + w.w0) % 16 == w.mis
                assert all((case.shift + p) % 16 == 0 for p in w.whole)


# ---- one deliberate fault per seam family: the restatement, changed the same way, predicts other bytes in the claiming case ------

def _windows_of_rows(case):
    a = rc.analysis(case)
    return {v: t.windows for t in a.tiles for v in range(t.t0, t.t1)}, a


def _gp_text_lost(case, front=0, behind=0):
    """bytes of 8-byte GP values that no window writes when gp_put skips a value on pos + 8 <= w0 + front || pos >= w1 - behind"""
    windows, a = _windows_of_rows(case)
    lost = 0
    for kind, p, i, v, s, e, b in a.spans:
        if kind == "gp" and len(b) == 8:
            got = set()
            for w in windows[v]:
                if not (s + 8 <= w.w0 + front or s >= w.w1 - behind):
                    got |= set(range(max(s, w.w0), min(e, w.w1)))
            lost += 8 - len(got)
    return lost


def test_fault_gp_put_skip_off_by_one():
    case = BY_NAME["text-gp-split"]
    assert _gp_text_lost(case) == 0
    assert _gp_text_lost(case, front=1) > 0, "gp-split-7: the value's last byte alone lies in the next window"
    assert _gp_text_lost(case, behind=1) > 0, "gp-split-1: the value's first byte alone lies in this window"
    # (narrowed by a byte the skip only lets a value through whose bytes FmtWindow::put then drops: no byte changes, nothing to catch)
    assert _gp_text_lost(case, front=-1) == 0 and _gp_text_lost(case, behind=-1) == 0


def _gp_bcf_lost(case, round_up=3):
    """bytes of a plane's GP floats that no window writes when put_gp ends a window's values at (w1 - at + round_up) / 4"""
    a = rc.analysis(case)
    lost = 0
    for kind, p, s, e in a.blocks():
        if kind != "gp":
            continue
        G, got = (e - s) // 4, set()
        t = next(t for t in a.tiles if t.b0 <= s < t.b1)
        for w in t.windows:
            if s >= w.w1 or e <= w.w0:
                continue
            g_lo = (w.w0 - s) // 4 if w.w0 > s else 0
            g_hi = (w.w1 - s + round_up) // 4 if w.w1 - s < G * 4 else G
            for g in range(g_lo, g_hi):
                got |= set(range(max(s + 4 * g, w.w0), min(s + 4 * g + 4, w.w1)))
        lost += (e - s) - len(got)
    return lost


def test_fault_put_gp_g_hi_rounds_short():
    case = BY_NAME["bcf-split"]
    assert _gp_bcf_lost(case) == 0
    assert _gp_bcf_lost(case, round_up=2) > 0, "bcf-split-4@1-gp: the float's first byte alone lies in this window"
    assert _gp_bcf_lost(BY_NAME["bcf-gp-window-dip"]) == 0 and _gp_bcf_lost(BY_NAME["bcf-gp-window-hap"]) == 0


def test_fault_a_correction_behind_the_square_root_dropped():
    """With a correctly rounded root neither loop ever runs below 2^50 values, so dropping one changes no byte at any size a test can
    reach: argued, not caught.  What the claimed seams pin is the other half: at g_lo = T(k) a root one ulp low needs the upward loop,
    at T(k) - 1 a root that is high needs the downward one; the cases put a window's first value on both, where a wrong (j, k) reads
    another value of the record (the cases' values are all different)."""
    exact = {rc.triangle(k) + j: (j, k) for k in range(110) for j in range(k + 1)}
    for g, jk in exact.items():
        assert rc.gp_jk(g) == rc.gp_jk(g, drop="up") == rc.gp_jk(g, drop="down") == jk
    low = lambda x: math.nextafter(math.sqrt(x), 0.0)
    high = lambda x: math.sqrt(x) * (1 + 2.0 ** -12)
    case = BY_NAME["bcf-gp-window-dip"]
    assert case.rows[-1].A == 101 and len(set(case.rows[-1].gp[0])) == case.rows[-1].G
    for k in (1, 2, 100):
        assert "gp-window-at-T%d+0-dip" % k in case.seams and "gp-window-at-T%d-1-dip" % k in case.seams
        g = rc.triangle(k)
        assert rc.gp_jk(g, root=low) == exact[g] and rc.gp_jk(g, root=low, drop="up") != exact[g]
        assert rc.gp_jk(g - 1, root=high) == exact[g - 1]
    assert rc.gp_jk(rc.triangle(100) - 1, root=high, drop="down") != exact[rc.triangle(100) - 1]


def test_fault_a_threshold_of_fmt_int_len_moved():
    ints = [int(b) for kind, p, i, v, s, e, b in BY_NAME["text-pow10"].spans() if kind in ("gt1", "gt2", "gq", "covs", "pl") and b != b"."]
    assert all(rc.int_len(x) == len(str(x)) for x in ints)
    for i, t in enumerate(rc.INT_THRESHOLDS):
        for moved in (t + 1, t - 1):
            mutant = rc.INT_THRESHOLDS[:i] + (moved,) + rc.INT_THRESHOLDS[i + 1:]
            assert any(rc.int_len(x, mutant) != len(str(x)) for x in ints), t
    info = [int(b) for kind, p, i, v, s, e, b in BY_NAME["info-pow10"].spans() if kind in ("ac", "an", "ns")]
    assert {len(str(x)) for x in info} >= set(range(1, 13))                     # (site_u64_len has no thresholds: a loop; every length to 12 digits)


def test_fault_flush_stores_a_whole_piece_in_front_of_the_window():
    """the faulty flush writes LDS bytes in front of w0: over the previous tile's last bytes or, for the first tile of a shifted buffer,
    in front of the buffer -- never run on the device"""
    case = BY_NAME["text-mis-all"]
    off = case.row_off()
    in_front = lambda tiles: sum(max(0, w.w0 - p) for t in tiles for w in t.windows for p in w.whole)
    assert in_front(rc.geometry(off, case.shift, case.total())) == 0
    assert in_front(rc.geometry(off, case.shift, case.total(), fault="flush-below-lo")) == sum(range(16))
    shifted = BY_NAME["text-window-full"]
    assert rc.store_map(rc.geometry(shifted.row_off(), shifted.shift, shifted.total(), fault="flush-below-lo"), shifted.total())[2] == shifted.shift


def test_fault_a_32_bit_carry_in_the_rescan():
    for n in rc.SCAN_N:
        for name, lens in rc.scan_inputs(n):
            want = [0] + list(itertools.accumulate(int(x) for x in lens))
            off, total = rc.scan_model(lens)
            assert off == want and total == want[-1], (n, name)
            bad = rc.scan_model(lens, carry_bits=32)[0]
            crosses = any(want[r] >= 1 << 32 for r in range(rc.SCAN_TPB, n + 1, rc.SCAN_TPB)) or want[-1] >= 1 << 32
            assert (bad != want) == crosses, (n, name)
    assert {name for name, _ in rc.scan_inputs(16385)} == {"all-max", "random"} | {"one-max-" + s for s in rc.SCAN_SPOTS}
