"""The case table of the IBS0-free segments (tests/ibd_model.py): directed cases at every seam of the walk -- the bits of a word, the words
of a chunk, the chunks of a run, the chromosomes, the two thresholds, the groups of samples, the cell rule -- and random cases.  A case is
a dict: name, n_samples, words (uint64 [groups, 3, n_vars], what mg_ibd_step takes), D (the same cells as dosages, -1: no contribution),
chrom, pos, min_records, min_bp, cuts (a list of lists of record indexes where a new step starts), expect (the table of the pair (0, 1) as
tuples (chrom, start_pos, end_pos, n, ibs2), or None where the model alone says) and seam (a function of the case that is true when the
case's input really has the property its name claims).  tests/test_ibd_cases_cpu.py proves both on the CPU."""
import numpy as np

from ibd_model import dosage_from_words
from ld_model import site_words, words_from_dosage

MIN_GQ = 30
# a record of a two-sample case: '=' both dosage 0 (CONC, IBS2), 'h' dosages 0 and 1 (CONC, not IBS2), 'x' dosages 0 and 2 (DISC),
# 'X' dosages 2 and 0 (DISC), '.' the first cell does not contribute (NEUT), ':' neither does
SYMBOLS = {"=": (0, 0), "h": (0, 1), "x": (0, 2), "X": (2, 0), ".": (-1, 0), ":": (-1, -1), "2": (2, 2), "1": (1, 1)}


def _case(name, D, n_samples, chrom=None, pos=None, min_records=1, min_bp=0, cuts=((),), expect=None, seam=None, words=None):
    D = np.asarray(D, dtype=np.int64).reshape(-1, n_samples)
    n = D.shape[0]
    chrom = np.zeros(n, dtype=np.uint32) if chrom is None else np.asarray(chrom, dtype=np.uint32)
    pos = (np.arange(n, dtype=np.uint32) * 10 + 100) if pos is None else np.asarray(pos, dtype=np.uint32)
    assert chrom.shape == (n,) and pos.shape == (n,)
    if words is None:
        words = words_from_dosage(D) if n_samples else None
    cuts = [sorted(c) for c in cuts]
    assert all(0 <= x <= n for c in cuts for x in c)
    case = dict(name=name, n_samples=n_samples, words=words, D=D, chrom=chrom, pos=pos, min_records=min_records, min_bp=min_bp, cuts=cuts, expect=expect,
                seam=seam or (lambda c: True))
    for x in (words, D, chrom, pos):
        x.setflags(write=False)
    return case


def _two(name, pattern, **kw):
    return _case(name, [SYMBOLS[s] for s in pattern], 2, **kw)


def _kind(c, v, a=0, b=1):
    da, db = int(c["D"][v, a]), int(c["D"][v, b])
    if da < 0 or db < 0:
        return "NEUT"
    return "DISC" if abs(da - db) == 2 else "CONC"


def _p(v):
    return 100 + 10 * v                              # the default position of record v


def _cells_case(name, g1, g2, gq, alleles, haploid, min_gq, **kw):
    """two samples from cells, by the rule of mg_pack_site_dosage (ld_model.site_words)"""
    g1, g2, gq = (np.asarray(x, dtype=np.int32).T.copy() for x in (g1, g2, gq))       # -> [samples, records]
    vao = np.zeros(len(alleles) + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(alleles)
    words = site_words(g1, g2, gq, haploid, vao, min_gq)[None]
    return _case(name, dosage_from_words(words, 2), 2, words=words, **kw)


def _group_case(n_samples, n=200, seed=7):
    """sample s is homozygous for the other allele at the records v with (v + 3 s) % 11 == 0, a few cells are heterozygous or out: every
    pair has several segments, the pairs inside a group and those across groups alike"""
    rng = np.random.default_rng(seed + n_samples)
    D = np.zeros((n, n_samples), dtype=np.int64)
    for s in range(n_samples):
        D[:, s] = np.where((np.arange(n) + 3 * s) % 11 == 0, 2, 0)
    D[rng.random((n, n_samples)) < 0.05] = 1
    D[rng.random((n, n_samples)) < 0.03] = -1

    def seam(c):
        from ibd_model import ibd_segments
        seg = ibd_segments(c["D"], c["chrom"], c["pos"], n_samples, 3, 0)
        inside = ((seg["a"] // 64) == (seg["b"] // 64)).any()
        across = ((seg["a"] // 64) != (seg["b"] // 64)).any()
        last = ((seg["b"] == n_samples - 1)).any()
        return bool(inside and last and (across or n_samples <= 64) and c["words"].shape[0] == (n_samples + 63) // 64)
    return _case("samples_%d" % n_samples, D, n_samples, min_records=3, cuts=[[], [64, 128], [65]], seam=seam)


def directed_cases():
    out = []
    E = lambda *t: [tuple(x) for x in t]
    # ---- the bits of a word, the words of a chunk
    out.append(_two("disc_at_bit_0", "x" + "=" * 129, cuts=[[], [64], [1]], expect=E((0, _p(1), _p(129), 129, 129)),
                    seam=lambda c: _kind(c, 0) == "DISC"))
    out.append(_two("disc_at_bit_63", "=" * 63 + "x" + "=" * 66, cuts=[[], [64], [63]], expect=E((0, _p(0), _p(62), 63, 63), (0, _p(64), _p(129), 66, 66)),
                    seam=lambda c: _kind(c, 63) == "DISC" and _kind(c, 62) == "CONC" and _kind(c, 64) == "CONC"))
    out.append(_two("disc_last_of_chunk", "=" * 10 + "X" + "h" * 10, cuts=[[11], [11, 15], []], expect=E((0, _p(0), _p(9), 10, 10), (0, _p(11), _p(20), 10, 0)),
                    seam=lambda c: all(_kind(c, cut[0] - 1) == "DISC" for cut in c["cuts"][:2])))
    out.append(_two("opens_in_bit_63_closes_in_bit_0", "." * 63 + "=" + "x" + "." * 5, cuts=[[], [64]], expect=E((0, _p(63), _p(63), 1, 1)),
                    seam=lambda c: _kind(c, 63) == "CONC" and _kind(c, 64) == "DISC" and _kind(c, 62) == "NEUT"))
    out.append(_two("pieces_inside_one_word", "==x=hX:=.x2211", expect=E((0, _p(0), _p(1), 2, 2), (0, _p(3), _p(4), 2, 1), (0, _p(7), _p(7), 1, 1), (0, _p(10), _p(13), 4, 4)),
                    cuts=[[], [3], [5, 6]]))
    # ---- the chunks of a run
    out.append(_two("run_across_three_chunks", "=" * 200, cuts=[[64, 128], [50, 150], [65, 130], []], expect=E((0, _p(0), _p(199), 200, 200)),
                    seam=lambda c: all(len(cut) == 2 for cut in c["cuts"][:3])))
    out.append(_two("neut_chunk_between_conc_chunks", "=" * 5 + ":" * 5 + "h" * 5, cuts=[[5, 10], []], expect=E((0, _p(0), _p(14), 10, 5)),
                    seam=lambda c: all(_kind(c, v) == "NEUT" for v in range(5, 10))))
    out.append(_two("empty_steps_between", "==" + "==", cuts=[[2, 2, 2], [0, 0, 4, 4], []], expect=E((0, _p(0), _p(3), 4, 4))))
    # ---- the chromosomes
    out.append(_two("chrom_change_at_a_chunks_first_record", "=" * 10, chrom=[0] * 5 + [1] * 5, cuts=[[5], [], [4], [6]],
                    expect=E((0, _p(0), _p(4), 5, 5), (1, _p(5), _p(9), 5, 5)), seam=lambda c: c["chrom"][4] != c["chrom"][5] and c["cuts"][0] == [5]))
    out.append(_two("chrom_change_on_a_neut_record", "==.==", chrom=[0, 0, 1, 1, 1], cuts=[[], [2], [3]], expect=E((0, _p(0), _p(1), 2, 2), (1, _p(3), _p(4), 2, 2)),
                    seam=lambda c: _kind(c, 2) == "NEUT" and c["chrom"][1] != c["chrom"][2]))
    out.append(_two("chrom_there_and_back_over_neut_records", "==:.==", chrom=[0, 0, 1, 1, 0, 0], cuts=[[], [2], [4], [2, 4]],
                    expect=E((0, _p(0), _p(1), 2, 2), (0, _p(4), _p(5), 2, 2)), seam=lambda c: c["chrom"][1] == c["chrom"][4] != c["chrom"][2]))
    out.append(_two("chrom_change_on_a_disc_record", "==x==", chrom=[0, 0, 1, 1, 1], cuts=[[], [2], [3]], expect=E((0, _p(0), _p(1), 2, 2), (1, _p(3), _p(4), 2, 2)),
                    seam=lambda c: _kind(c, 2) == "DISC" and c["chrom"][1] != c["chrom"][2]))
    out.append(_two("chrom_change_on_a_conc_record", "==h==", chrom=[7, 7, 9, 9, 9], cuts=[[], [2], [3]], expect=E((7, _p(0), _p(1), 2, 2), (9, _p(2), _p(4), 3, 2)),
                    seam=lambda c: _kind(c, 2) == "CONC" and c["chrom"][1] != c["chrom"][2]))
    # ---- the thresholds
    out.append(_two("min_records_exact_and_one_less", "===x==", min_records=3, cuts=[[], [3], [4]], expect=E((0, _p(0), _p(2), 3, 3))))
    out.append(_two("min_bp_exact_and_one_less", "==x==", pos=[100, 1100, 1200, 2000, 2999], min_bp=1000, cuts=[[], [2], [4]], expect=E((0, 100, 1100, 2, 2)),
                    seam=lambda c: c["pos"][1] - c["pos"][0] == c["min_bp"] and c["pos"][4] - c["pos"][3] == c["min_bp"] - 1))
    out.append(_two("equal_pos_length_0", "==", pos=[5, 5], min_bp=0, cuts=[[], [1]], expect=E((0, 5, 5, 2, 2))))
    out.append(_two("positions_at_the_top_of_32_bits", "=h", pos=[0, 0xFFFFFFFF], min_bp=0xFFFFFFFF, cuts=[[], [1]], expect=E((0, 0, 0xFFFFFFFF, 2, 1))))
    out.append(_two("positions_going_down", "==", pos=[500, 100], min_bp=0, cuts=[[], [1]], expect=E(), seam=lambda c: int(c["pos"][1]) - int(c["pos"][0]) < 0))
    # ---- the number of records
    for n in (0, 1, 63, 64, 65, 129):
        out.append(_two("n_vars_%d" % n, "=" * n, cuts=[[]] + ([[n // 2]] if n > 1 else []), expect=E((0, _p(0), _p(n - 1), n, n)) if n else E(),
                        seam=lambda c, n=n: c["D"].shape[0] == n))
    # ---- the samples and their groups
    for S in (2, 64, 65, 130):
        out.append(_group_case(S))
    # ---- the cell rule (mg_pack_site_dosage's, unchanged)
    hom_ref, hom_alt = (0, 0), (1, 1)
    g1 = [(0, 0), (0, 0), (0, 1), (0, 1), (0, 0), (0, 2), (0, -1), (0, 1), (0, 0)]      # [record](sample 0, sample 1)
    g2 = [(0, 0), (0, 0), (0, 1), (0, 1), (0, 0), (0, 1), (0, 1), (0, 1), (0, 0)]
    out.append(_cells_case("multi_allelic_and_out_of_range_are_neut", g1, g2, np.full((9, 2), 50), [2, 2, 3, 1, 2, 2, 2, 2, 2], False, None,
                           expect=E((0, _p(0), _p(4), 3, 3), (0, _p(8), _p(8), 1, 1)), cuts=[[], [3], [6]],
                           seam=lambda c: [_kind(c, v) for v in range(9)] == ["CONC", "CONC", "NEUT", "NEUT", "CONC", "NEUT", "NEUT", "DISC", "CONC"]))
    out.append(_cells_case("haploid", [(0, 0), (1, 1), (0, 1), (1, 1), (1, 0), (0, 0)], [(9, 9)] * 6, np.full((6, 2), 50), [2] * 6, True, None,
                           expect=E((0, _p(0), _p(1), 2, 2), (0, _p(3), _p(3), 1, 1), (0, _p(5), _p(5), 1, 1)), cuts=[[], [2]],
                           seam=lambda c: set(np.unique(c["D"])) == {0, 2}))
    g = [(0, 0), (0, 1), (0, 0), (0, 1), (0, 0)]
    out.append(_cells_case("gq_mask_both_sides", g, g, [(50, 50), (50, MIN_GQ - 1), (50, 50), (MIN_GQ, MIN_GQ), (50, 50)], [2] * 5, False, MIN_GQ,
                           expect=E((0, _p(0), _p(2), 2, 2), (0, _p(4), _p(4), 1, 1)), cuts=[[], [1], [3]],
                           seam=lambda c: [_kind(c, v) for v in range(5)] == ["CONC", "NEUT", "CONC", "DISC", "CONC"]))
    # ---- the flush
    out.append(_two("open_run_at_flush", "x===", cuts=[[], [2]], expect=E((0, _p(1), _p(3), 3, 3)), seam=lambda c: _kind(c, 3) == "CONC"))
    assert len({c["name"] for c in out}) == len(out)
    return out


# ---- random cases --------------------------------------------------------------------------------------------------------------------
# (n_samples, n_vars, min_records, seed): the seeds were chosen on the CPU so that the model alone emits a segment and filters a closed run
# by each threshold that can filter (min_records == 1 keeps nothing out) -- tests/test_ibd_cases_cpu.py asserts it
RANDOM = [(2, 3000, 5, 1), (17, 1500, 1, 2), (64, 1000, 5, 3), (65, 700, 1, 4), (130, 3000, 5, 5)]
RANDOM_MIN_BP = 1500


def random_case(n_samples, n_vars, min_records, seed):
    """dosages 0 / 1 / 2 at 80 / 16 / 4 % with 5 % of the cells out: a DISC rate of a few percent per pair, runs of tens of records; three
    chromosomes; positions 1 .. 200 apart"""
    rng = np.random.default_rng(seed)
    D = rng.choice(np.array([0, 1, 2, -1]), size=(n_vars, n_samples), p=[0.76, 0.15, 0.04, 0.05])
    chrom = np.sort(rng.integers(0, 3, size=n_vars)).astype(np.uint32)
    pos = np.cumsum(rng.integers(1, 201, size=n_vars)).astype(np.uint32)
    cuts = [[], list(range(64, n_vars, 64)), list(range(65, n_vars, 65)), list(range(1000, n_vars, 1000))]
    return _case("random_%d_%d_%d" % (n_samples, n_vars, min_records), D, n_samples, chrom=chrom, pos=pos, min_records=min_records, min_bp=RANDOM_MIN_BP, cuts=cuts)


# ---- seam cases: the chunks of ibd_walk_kernel, the words of ibd_starts_kernel, the tiles of pairs -------------------------------------------
# The same dicts as directed_cases(), with `seams`: the seams of IBD_SEAMS the case claims.  A step of more than 2,048 records takes a second
# trip through the kernel's chunk loop (PAIR_CHUNK = 32 words, staged with the chromosome-start words beside them); these cases put a
# break, an open run or a chromosome change on both sides of that trip, in one step and with cuts at the seam.
PAIR_CHUNK, PAIR_TILE, IBD_TR_WORDS = 32, 16, 16                        # pair_kernels.h, ibd_kernels.h (a test's copy)
CHUNK_RECORDS = 64 * PAIR_CHUNK


def _only_pair(S, a, b, pattern, n_front=0):
    """S samples, all cells missing but those of samples a and b, which carry the two-sample pattern"""
    D = np.full((n_front + len(pattern), S), -1, dtype=np.int64)
    for v, s in enumerate(pattern):
        D[n_front + v, a], D[n_front + v, b] = SYMBOLS[s]
    return D


def _counts_case(S, n=120):
    """sample s is hom-alt at the records v with v % (s + 2) == 0, hom-ref elsewhere: every pair is broken at places of its own, so the pairs'
    segment counts differ and the table is right only if every pair's segments lie at its own offset, in order"""
    v = np.arange(n)[:, None]
    D = np.where(v % (np.arange(S)[None, :] + 2) == 0, 2, 0).astype(np.int64)
    return _case("samples_%d_every_pair_its_own_count" % S, D, S, cuts=[[], [64], [50, 50, 100]], seam=lambda c: True)


def seam_cases():
    out = []
    E = lambda *t: [tuple(x) for x in t]
    C = CHUNK_RECORDS

    def add(seams, *a, **kw):
        c = _two(*a, **kw)
        c["seams"] = set(seams)
        out.append(c)
    # ---- the second trip through the chunk loop: records 2,047 / 2,048 and 4,095 / 4,096
    add({"step_2049", "disc_at_2047"}, "disc_last_of_the_first_trip", "=" * (C - 1) + "x" + "=", cuts=[[], [C], [C - 1]],
        expect=E((0, _p(0), _p(C - 2), C - 1, C - 1), (0, _p(C), _p(C), 1, 1)), seam=lambda c: _kind(c, C - 1) == "DISC" and len(c["D"]) == C + 1)
    add({"step_4096", "disc_at_2048"}, "disc_first_of_the_second_trip", "=" * C + "x" + "=" * (C - 1), cuts=[[], [C], [C + 1]],
        expect=E((0, _p(0), _p(C - 1), C, C), (0, _p(C + 1), _p(2 * C - 1), C - 1, C - 1)), seam=lambda c: _kind(c, C) == "DISC" and len(c["D"]) == 2 * C)
    add({"step_4097", "open_across_2047_2048", "open_across_4095_4096"}, "runs_open_across_both_trips", "." * (C - 8) + "h" * 16 + "." * (C - 16) + "=" * 9,
        cuts=[[], [C], [C, 2 * C], [2 * C]], expect=E((0, _p(C - 8), _p(2 * C), 25, 9)),                      # (NEUT records break nothing: one run, open across both seams)
        seam=lambda c: all(_kind(c, v) == "CONC" for v in (C - 1, C, 2 * C - 1, 2 * C)) and len(c["D"]) == 2 * C + 1)
    add({"step_2049", "opens_2047_closes_2048"}, "opens_last_of_the_first_trip_closes_first_of_the_second", "." * (C - 1) + "=" + "x", cuts=[[], [C]],
        expect=E((0, _p(C - 1), _p(C - 1), 1, 1)), seam=lambda c: _kind(c, C - 2) == "NEUT" and _kind(c, C - 1) == "CONC" and _kind(c, C) == "DISC")
    add({"step_2048"}, "one_full_trip", "x" + "=" * (C - 1), cuts=[[], [C]], expect=E((0, _p(1), _p(C - 1), C - 1, C - 1)), seam=lambda c: len(c["D"]) == C)
    add({"step_4096", "second_trip_neut_only"}, "second_trip_of_neut_records_only", "=" * C + ":" * C, cuts=[[], [C]], expect=E((0, _p(0), _p(C - 1), C, C)),
        seam=lambda c: all(_kind(c, v) == "NEUT" for v in range(C, 2 * C)))
    # ---- a chromosome change exactly at record 2,048 and at 4,096: the start words staged beside the chunk
    for sym, kind in (("=", "CONC"), ("x", "DISC"), (".", "NEUT")):
        open_at = 0 if kind == "CONC" else 1
        segs = [(0, _p(0), _p(C - 1), C, C), (1, _p(C + open_at), _p(2 * C - 1), C - open_at, C - open_at)] + ([(2, _p(2 * C), _p(2 * C), 1, 1)] if kind == "CONC" else [])
        add({"step_4097", "chrom_at_2048_" + kind, "chrom_at_4096_" + kind}, "chrom_change_first_of_each_later_trip_on_" + kind.lower(),
            "=" * C + sym + "=" * (C - 1) + sym, chrom=[0] * C + [1] * C + [2], cuts=[[], [C], [C, 2 * C]], expect=E(*segs),
            seam=lambda c, kind=kind: _kind(c, C) == kind and _kind(c, 2 * C) == kind and c["chrom"][C - 1] != c["chrom"][C] and c["chrom"][2 * C - 1] != c["chrom"][2 * C])
    # the start word of the second trip is not the first trip's: a change at record 2,048 + 69 alone, and -- the decoy -- one at record 69 alone
    k = C + 69
    add({"start_word_of_the_second_trip"}, "chrom_change_inside_the_second_trip_alone", "=" * (C + 200), chrom=[0] * k + [1] * (C + 200 - k), cuts=[[], [C]],
        expect=E((0, _p(0), _p(k - 1), k, k), (1, _p(k), _p(C + 199), C + 200 - k, C + 200 - k)), seam=lambda c: int(np.flatnonzero(np.diff(c["chrom"]))[0]) + 1 == C + 69)
    add({"start_word_decoy"}, "chrom_change_inside_the_first_trip_alone", "=" * (C + 200), chrom=[0] * 69 + [1] * (C + 131), cuts=[[], [C]],
        expect=E((0, _p(0), _p(68), 69, 69), (1, _p(69), _p(C + 199), C + 131, C + 131)), seam=lambda c: int(np.flatnonzero(np.diff(c["chrom"]))[0]) + 1 == 69)
    # ---- ibd_starts_kernel: a word a wave, four words a workgroup; record 0 of a step is compared with *last
    changes = [63, 64, 255, 256, 512]
    chrom = np.searchsorted(changes, np.arange(600), side="right")
    edges = [0] + changes + [600]
    add({"starts_63_64", "starts_255_256", "starts_256k", "change_after_an_empty_step", "last_over_two_empty_steps"}, "chrom_changes_at_word_and_workgroup_seams", "=" * 600,
        chrom=chrom, cuts=[[], [64], [256], [256, 256], [256, 256, 256, 512], [63, 255]],
        expect=E(*[(i, _p(lo), _p(hi - 1), hi - lo, hi - lo) for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:]))]),
        seam=lambda c: [int(x) + 1 for x in np.flatnonzero(np.diff(c["chrom"]))] == changes and [256, 256] in c["cuts"] and [256, 256, 256, 512] in c["cuts"])
    # ---- break words
    add({"breaks_0_63_neighbours"}, "breaks_at_bit_0_and_at_two_neighbouring_bits_62_63", "x" + "=" * 61 + "xX" + "=" * 64, cuts=[[], [63], [64]],
        expect=E((0, _p(1), _p(61), 61, 61), (0, _p(64), _p(127), 64, 64)), seam=lambda c: [_kind(c, v) for v in (0, 62, 63)] == ["DISC"] * 3)
    add({"start_and_disc"}, "a_record_that_starts_a_chromosome_and_is_disc", "=" * 64 + "x" + "=" * 5, chrom=[0] * 64 + [1] * 6, cuts=[[], [64]],
        expect=E((0, _p(0), _p(63), 64, 64), (1, _p(65), _p(69), 5, 5)), seam=lambda c: _kind(c, 64) == "DISC" and c["chrom"][63] != c["chrom"][64])
    add({"word_of_disc"}, "a_whole_word_of_disc_then_a_whole_word_of_conc", "h" * 64 + "x" * 64 + "=" * 64, cuts=[[], [64], [128]],
        expect=E((0, _p(0), _p(63), 64, 0), (0, _p(128), _p(191), 64, 64)), seam=lambda c: all(_kind(c, v) == "DISC" for v in range(64, 128)))
    # ---- the tiles of pairs: exactly one pair has segments, every other sample is missing throughout
    pattern = "==x=h=X=="
    for S in (15, 16, 17, 31, 32, 33):
        for a, b in sorted({(0, 15), (15, 16), (0, 16), (16, 17), (S - 2, S - 1)}):
            if b >= S:
                continue
            c = _case("samples_%d_only_pair_%d_%d" % (S, a, b), _only_pair(S, a, b, pattern), S, cuts=[[], [3]], seam=lambda c: True)
            c["seams"], c["only"] = {"samples_%d" % S}, (a, b)
            if (a, b) in ((0, 15), (15, 16), (0, 16), (16, 17)):
                c["seams"].add("only_pair_%d_%d" % (a, b))
            if (a, b) == (S - 2, S - 1):
                c["seams"].add("only_pair_last_pair")
            out.append(c)
        c = _counts_case(S)
        c["seams"] = {"samples_%d" % S, "all_pairs_%d" % S}
        out.append(c)
    assert len({c["name"] for c in out}) == len(out)
    return out


IBD_SEAMS = ({"step_2048", "step_2049", "step_4096", "step_4097", "disc_at_2047", "disc_at_2048", "open_across_2047_2048", "open_across_4095_4096", "opens_2047_closes_2048",
              "second_trip_neut_only", "start_word_of_the_second_trip", "start_word_decoy", "starts_63_64", "starts_255_256", "starts_256k", "change_after_an_empty_step",
              "last_over_two_empty_steps", "breaks_0_63_neighbours", "start_and_disc", "word_of_disc", "only_pair_0_15", "only_pair_15_16", "only_pair_0_16", "only_pair_16_17",
              "only_pair_last_pair"} | {"chrom_at_%d_%s" % (v, k) for v in (2048, 4096) for k in ("CONC", "DISC", "NEUT")} |
             {"samples_%d" % s for s in (15, 16, 17, 31, 32, 33)} | {"all_pairs_%d" % s for s in (15, 16, 17, 31, 32, 33)})

# the transpose: one cell, and the decoy the same bit one record and one sample on, in the next dosage row: two bits come out, nothing else
TR_SAMPLES, TR_N = (0, 1, 62, 63, 64, 127, 129), 1100
TR_RECORDS = (0, 63, 64, 255, 256, 1023, 1024, TR_N - 1)


def transpose_case(sample, record, decoy=True):
    """-> (words [3, 3, 1100], planes [192, 3, 18]): the input and what must come out, written down bit by bit"""
    words, planes = np.zeros((3, 3, TR_N), dtype=np.uint64), np.zeros((192, 3, (TR_N + 63) // 64), dtype=np.uint64)
    d = (sample + record) % 3
    cells = [(sample, d, record)] + ([((sample + 1) % 130, (d + 1) % 3, (record + 1) % TR_N)] if decoy else [])
    for s, dd, v in cells:
        words[s // 64, dd, v] |= np.uint64(1) << np.uint64(s % 64)
        planes[s, dd, v // 64] |= np.uint64(1) << np.uint64(v % 64)
    return words, planes
