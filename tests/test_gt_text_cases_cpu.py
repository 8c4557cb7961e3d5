"""tests/gt_text_cases.py holds what it says, checked from the bytes and without a GPU: every tab sits on the seam its case names,
every span has its length, the record counts pass the two grids, the default-word cases count what they claim, and the model
reads every case.  The same GT forms then go through the HOST decoder (VcfReader::parse_samples, the comparator of the device
path in tests/test_gpu_cli.py and its fall-back for allele numbers above 127) against the model, through `dump-kmers`."""
import numpy as np
import pytest

import gt_call_panels as gcp
import gt_text_cases as gtc
import vcf_synth
from oracle import pipeline
from test_host_enumerator_cpu import cli_dump, oracle_dump


@pytest.fixture(scope="module")
def call_panel(tmp_path_factory):
    return gcp.call_panel(str(tmp_path_factory.mktemp("call_panel") / "p"))


@pytest.mark.parametrize("name", list(gtc.CASES))
def test_case_holds_its_claims_and_the_model_reads_it(tmp_path, name):
    case = gtc.get(name)
    seen = gtc.check_claims(case, str(tmp_path))
    assert "records" in seen and len(seen) >= 2, "a case that claims nothing about its bytes"
    for haploid in case.modes:
        b = gtc.build(case, str(tmp_path), haploid)
        assert len(b.want) == len(b.off) == len(b.select)
        assert all(len(w) == b.n_keep for w in b.want)
        if haploid:
            assert all(int(w.min()) >= gtc.PHASED0 for w in b.want if len(w))
        dflt = gtc.claim(case, "default")
        if dflt is not None and not haploid:
            assert gtc.default_word(b.want, False) == dflt[0]            # the model's words agree with what the bytes were counted to give


def _tabs(name):
    return [(c[1], c[2]) for c in gtc.get(name).claims if c[0] == "tab"]


@pytest.mark.parametrize("sfx", ["-gt-in-front", "-gt-behind"])
def test_scan_seams_are_hit(sfx):
    """a tab as the last and as the first byte of a piece of 16, of a wave's 1,024 and of a tile's 4,096, with no tab on the seam's other side"""
    for where, res in (("last", -1), ("first", 0)):
        name = "A-tab-%s-of-piece-wave-tile%s" % (where, sfx)
        tabs = _tabs(name)
        offs = {o for _, o in tabs}
        for unit in (gtc.PIECE, gtc.WAVE_BYTES, gtc.TILE):
            assert [o for o in offs if o % unit == res % unit], (name, unit)
        for r, o in tabs:
            other = o + 1 if res else o - 1                              # the byte across the seam is no tab
            if o % gtc.PIECE == res % gtc.PIECE:
                assert (r, other) not in tabs, (name, r, o)
        assert {o for o in offs if o % gtc.TILE == res % gtc.TILE and o > gtc.TILE}, "the seam between the second and third tile"
    lens = {c[2] for c in gtc.get("A-span-lengths" + sfx).claims if c[0] == "span_len"}
    assert lens == set(gtc.SPAN_LENGTHS)


def test_the_other_geometry_cases_are_what_they_name():
    sixteen = gtc.get("A-sixteen-tabs")
    for r in range(len(sixteen.records)):
        offs = sorted(o for rr, o in _tabs("A-sixteen-tabs") if rr == r)
        runs = [o for o in offs if o % gtc.PIECE == 0 and all(o + b in offs for b in range(gtc.PIECE))]
        assert runs, r
    assert {min(o for rr, o in _tabs("A-sixteen-tabs") if rr == r and o % gtc.PIECE == 0) % gtc.TILE for r in range(len(sixteen.records))} >= {0, gtc.TILE - gtc.PIECE}
    blank = [c for c in gtc.get("A-tile-without-tab").claims if c[0] == "no_tab"]
    assert len(blank) == 4
    for _, r, a, b in blank:
        lo = (a + gtc.TILE - 1) // gtc.TILE * gtc.TILE
        assert lo + gtc.TILE <= b, "no whole tile inside the column"
    assert [g for g in gtc.get("A-tile-without-tab").fmts] == ["GT:XX", "XX:GT", "GT:XX", "XX:GT"]
    edge = _tabs("A-edge-tabs")
    assert (0, 0) in edge and (1, -1) in edge and (2, 0) in edge and (2, -1) in edge
    five = gtc.get("A-five-tiles")
    assert gtc.claim(five, "records") == (2,) and [c for c in five.claims if c[0] == "span_len"][0][2] > 4 * gtc.TILE


def test_widths_masks_and_compaction_seam():
    for n in gtc.WIDTHS:
        assert gtc.get("B-width-%d" % n).n_columns == n and gtc.get("B-width-%d" % n).keep is None
    for n in (300, 513):
        kept = {kind: np.flatnonzero(gtc.get("B-keep-%d-%s" % (n, kind)).keep).tolist() for kind in gtc.KEEP_MASKS}
        assert kept["first"] == [0] and kept["last"] == [n - 1] and kept["middle"] == [n // 2] and kept["alternate"] == list(range(0, n, 2))
    for name in ("B-compact-seam", "B-compact-seam-alternate-kept"):
        odd = [c[2] for c in gtc.get(name).claims if c[0] == "odd_kept"]
        assert [gtc.COMPACT_TILE - 1] in odd and [gtc.COMPACT_TILE] in odd and [gtc.COMPACT_TILE + 1] in odd and [] in odd


def test_record_counts_pass_both_grids_and_neighbours_in_a_workgroup_differ():
    assert set(gtc.RECORD_COUNTS) >= {g + d for g in (gtc.DECODE_GRID, gtc.COMPACT_GRID) for d in (-1, 0, 1)}
    for name in ["C-records-%d" % n for n in gtc.RECORD_COUNTS] + ["C-records-1100-wide-300"]:
        case = gtc.get(name)
        recs = case.records
        n_keep = case.n_columns if case.keep is None else int(case.keep.sum())
        for grid in (1, gtc.DECODE_GRID, gtc.COMPACT_GRID):
            pairs = [(r - grid, r) for r in range(grid, len(recs))]
            if grid > 1 and len(recs) > grid:
                assert pairs
            for a, b in pairs:
                if recs[a] is None and recs[b] is None:
                    continue
                assert recs[a] != recs[b], (name, a, b)
                if grid > 1:                                             # what one workgroup takes in turn: another kind of record
                    assert gtc.loop_kind(a) != gtc.loop_kind(b), (name, a, b)
        short = [r for r, c in enumerate(recs) if c is not None and len(c) < case.n_columns]
        none = [r for r, c in enumerate(recs) if c is None]
        assert none == list(range(4, len(recs), 5))
        assert short == [r for r in range(2, len(recs), 3) if r % 5 != 4]
        if len(recs) > gtc.DECODE_GRID + 10:                             # a short record whose workgroup held a full one the turn before
            assert any(recs[r - gtc.DECODE_GRID] is not None and len(recs[r - gtc.DECODE_GRID]) == case.n_columns for r in short if r >= gtc.DECODE_GRID)
        if name == "C-records-1100-wide-300":
            assert n_keep > gtc.COMPACT_TILE and len(recs) > gtc.DECODE_GRID
        else:
            assert n_keep == 3
    assert gtc.LOOP_TWICE == ("C-records-3100", "C-records-1025")


def test_default_word_cases_count_what_they_claim():
    want = {"F-phased-one-more": (1, gtc.PHASED0), "F-tie": (0, gtc.PHASED0), "F-phased-one-fewer": (-1, 0)}
    for name, (diff, dflt) in want.items():
        p0, u0 = gtc.claim(gtc.get(name), "zero_words")
        assert p0 - u0 == diff and gtc.claim(gtc.get(name), "default") == (dflt,)
    p0, u0 = gtc.claim(gtc.get("F-only-unphased"), "zero_words")
    assert p0 == 0 and u0 == 6 * 5 and gtc.claim(gtc.get("F-only-unphased"), "default") == (0,)


def test_largest_allele_case(tmp_path):
    case = gtc.get("E-largest-allele")
    b = gtc.build(case, str(tmp_path), False)
    beyond = set(gtc.claim(case, "max_only")[0])
    assert len(beyond) == 9
    got = sorted({m for r, m in enumerate(b.maxes) if r not in beyond and m > 3})
    assert got == [128, 32767]                                           # what the model is asked about; past it the device reports 32,767
    assert dict(zip(gtc.BIG_ALLELES, gtc.BIG_MAX)) == {a: min(int(a), 32767) for a in gtc.BIG_ALLELES}


def test_token_forms_sit_first_middle_and_last(tmp_path):
    for name, kept in (("D-forms", [0, 1, 2, 3, 4]), ("D-forms-kept-3-of-7", [1, 3, 5])):
        case = gtc.get(name)
        where = {}
        for (_, r, odd), cells in zip([c for c in case.claims if c[0] == "odd_kept"], case.records):
            assert len(odd) == 1
            where.setdefault(cells[kept[odd[0]]], set()).add((odd[0], cells[kept[odd[0]] - 1 if odd[0] else kept[1]]))
        assert set(where) == set(gtc.FORMS)
        for f, at in where.items():
            assert at == {(s, fill) for s in (0, len(kept) // 2, len(kept) - 1) for fill in ("1|2", "3")}, f
    assert len(gtc.LONG_GT.split("|")) == 300
    assert {gtc.claim(gtc.get("D-gt-index-%d" % g), "records") for g in (0, 1, 5, gtc.MAX_GT_INDEX)} == {(4,)}


def test_refusals_spoil_a_valid_batch(tmp_path):
    b = gtc.build(gtc.get(gtc.REFUSALS_OVER), str(tmp_path), False)
    for name, spoil in gtc.REFUSALS.items():
        a = dict(raw=b.raw, off=b.off, ln=b.ln, gi=b.gi, n_columns=b.n_columns, keep=b.keep)
        spoil(a)
        changed = [k for k in a if a[k] is not getattr(b, k)]
        assert changed, name
    assert int(b.off[-1]) + int(b.ln[-1]) <= len(b.raw)


def test_call_panel_is_what_the_cli_cases_need(call_panel):
    """tests/test_gpu_cli.py's panel: wide enough for the device path by itself, more records in one block of text than either grid,
    runs whose every cut batch has its own commonest zero word, two records of 130 ALT alleles carrying 127, 128 and 129"""
    raw, off, ln, gi = gtc._spans(call_panel.prefix + ".vcf")
    assert len(off) == gcp.CALL_RECORDS >= 2100 > gtc.COMPACT_GRID and gcp.CALL_SAMPLES >= 1024
    assert int(ln.astype(np.int64).sum()) < 16 << 20 and int(ln.min()) > 4000
    assert gcp.CALL_RUN % gcp.CALL_CUT_BATCH == 0
    for a in range(0, len(off), gcp.CALL_CUT_BATCH):
        text = b"\t".join(raw[int(off[r]):int(off[r]) + int(ln[r])] for r in range(a, min(a + gcp.CALL_CUT_BATCH, len(off))))
        cols = text.split(b"\t")
        p0, u0 = cols.count(b"0|0"), cols.count(b"0/0")
        assert (p0 > 20 * u0) if (a // gcp.CALL_RUN) % 2 else (u0 > 20 * p0), a
    lines = [l for l in raw.split(b"\n") if l and not l.startswith(b"#")]
    pos = [(l.split(b"\t", 2)[0], int(l.split(b"\t", 2)[1])) for l in lines]
    for v, clustered in ((call_panel.wide_lone, False), (call_panel.wide_clustered, True)):
        f = lines[v].split(b"\t")
        assert f[4].count(b",") == gcp.WIDE_ALTS - 1 and len(set(f[4].split(b",") + [f[3]])) == gcp.WIDE_ALTS + 1
        alleles = {int(t) for g in f[9:] for t in g.replace(b"/", b"|").split(b"|")}
        assert {127, 128, 129} <= alleles and max(alleles) == gcp.WIDE_ALTS - 1
        near = min(abs(pos[w][1] - pos[v][1]) for w in (v - 1, v + 1) if pos[w][0] == pos[v][0])
        assert (near <= 17) if clustered else (near > 40)
        assert v // gcp.CALL_CUT_BATCH == (v - 1) // gcp.CALL_CUT_BATCH == (v + 1) // gcp.CALL_CUT_BATCH      # (its neighbours share its decode call)
    assert f[9 + gcp.CALL_SAMPLES - 1] == gcp.WIDE_GTS[gcp.CALL_SAMPLES - 1].encode()


def test_plain_call_panel_differs_in_the_two_wide_records_only(call_panel, tmp_path):
    plain = gcp.call_panel(str(tmp_path / "p"), wide=False)
    a = open(call_panel.prefix + ".vcf").read().split("\n")
    b = open(plain.prefix + ".vcf").read().split("\n")
    first = next(i for i, l in enumerate(a) if l and not l.startswith("#"))
    assert len(a) == len(b) and [i - first for i in range(len(a)) if a[i] != b[i]] == [call_panel.wide_lone, call_panel.wide_clustered]
    assert all(l.split("\t")[4].count(",") == 0 for l in b[first:] if l)   # no record that would send a batch to the host enumerator


def test_beyond_panel(tmp_path):
    prefix = str(tmp_path / "b")
    lines, at = gcp.beyond_panel(prefix)
    for allele in (None,) + gcp.BEYOND_ALLELES:
        seq, pos = gcp.write_beyond(prefix, lines, at, allele)
        raw, off, ln, gi = gtc._spans(prefix + ".vcf")
        assert len(off) == gcp.BEYOND_RECORDS
        f = raw.split(b"\n")[at].split(b"\t")
        assert (f[0].decode(), int(f[1])) == (seq, pos) and f[4].count(b",") == 1 and len(f) == 9 + gcp.CALL_SAMPLES
        assert f[9 + gcp.BEYOND_SAMPLE] == ("%s|0" % (allele or "2")).encode()
        assert (allele is None) == all(int(t) <= 2 for g in f[9:] for t in g.split(b"|"))


# ---- the host decoder on the same forms ---------------------------------------------------------------------------------------
def _panel_with_forms(prefix, seed, haploid):
    """vcf_synth.make_case with its GT columns replaced by family D's forms, allele numbers inside each record's kept ALT list"""
    vcf_synth.make_case(prefix, seed, haploid=haploid, n_samples=7)
    rng = np.random.default_rng(seed)
    out, used = [], set()
    for line in open(prefix + ".vcf").read().split("\n"):
        if line and not line.startswith("#"):
            f = line.split("\t")
            n_alt = sum(1 for a in f[4].split(",") if not a.startswith("<"))
            ok = [g for g, big in gtc.PANEL_FORMS if big <= n_alt]
            kind = len(out) % 3
            if kind == 0:                                                # ploidy 1 throughout
                ok = [g for g in ok if "|" not in g and "/" not in g]
            f[9:] = [ok[int(i)] for i in rng.integers(0, len(ok), size=len(f) - 9)]
            if kind == 2 and n_alt >= 1:                                 # one form among ploidy-1 neighbours
                f[9:] = ["1"] * (len(f) - 9)
                f[9 + int(rng.integers(0, len(f) - 9))] = ok[int(rng.integers(0, len(ok)))]
            used.update(f[9:])
            line = "\t".join(f)
        out.append(line)
    with open(prefix + ".vcf", "w") as fh:
        fh.write("\n".join(out))
    assert used == {g for g, _ in gtc.PANEL_FORMS}
    return prefix + ".fa", prefix + ".vcf"


@pytest.mark.parametrize("haploid", [False, True])
def test_host_decoder_reads_the_forms_as_the_model_does(tmp_path, haploid):
    fa, vcf = _panel_with_forms(str(tmp_path / "forms"), 31 + haploid, haploid)
    opt = pipeline.Options(haploid=haploid)
    for for_index in (True, False):
        want = oracle_dump(fa, vcf, opt, for_index)
        assert want.count("BLOCK") > 30 and "SIG 2 " in want
        for pool in (0, 1):
            assert cli_dump(fa, vcf, opt, for_index, pool=pool) == want, (for_index, pool)


@pytest.mark.parametrize("allele", gcp.BEYOND_ALLELES + ("99999999999999999999999",))
def test_host_decoder_does_not_fold_a_huge_allele_number_into_the_alt_list(tmp_path, allele):
    """parse_samples saturates as gt_column does on the device: 4294967296 is not allele 0, 2147483648 not a negative number, 23 digits
    no overflow -- the enumerator meets an allele the record does not have and stops, where it lists the k-mers of `2|0`"""
    import os
    import subprocess
    from test_host_enumerator_cpu import BIN
    prefix = str(tmp_path / "b")
    lines, at = gcp.beyond_panel(prefix)
    for a, refused in ((None, False), (allele, True)):
        gcp.write_beyond(prefix, lines, at, a)
        for mode in ("index", "call"):
            for pool in ("0", "1"):
                r = subprocess.run([BIN, "dump-kmers", "-k", "35", "-r", "43", prefix + ".fa", prefix + ".vcf", mode], capture_output=True, text=True, timeout=600,
                                   env=dict(os.environ, MALVA_GENO_VCF_POOL=pool))
                assert (r.returncode != 0) == refused, (a, mode, pool, r.stderr[-500:])
