"""The case table of the IBS0-free segments (tests/ibd_cases.py) proved on the CPU: every directed case has the property its name claims and
the table written beside it by hand, and the restatement (tests/ibd_model.py) gives the same table however the records are cut into steps.
The random cases emit and filter what tests/test_gpu_ibd.py relies on."""
import numpy as np
import pytest

import ibd_cases
from ibd_model import IBD_SEG, IbdModel, dosage_from_words, ibd_segments, planes_from_words, sort_segments

CASES = ibd_cases.directed_cases()


def _whole(c, cuts=()):
    return ibd_segments(c["D"], c["chrom"], c["pos"], c["n_samples"], c["min_records"], c["min_bp"], cuts=cuts)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_a_directed_case_hits_its_seam_and_does_not_depend_on_the_cuts(case):
    assert case["seam"](case), "the case does not have the property it names"
    assert np.array_equal(dosage_from_words(case["words"], case["n_samples"]), case["D"]), "words and dosages are the same cells"
    whole = _whole(case)
    if case["expect"] is not None:
        assert case["n_samples"] == 2
        assert [tuple(int(s[f]) for f in ("chrom", "start_pos", "end_pos", "n", "ibs2")) for s in whole] == case["expect"]
    assert not whole["zero"].any() and (whole["a"] < whole["b"]).all()
    key = whole["a"].astype(np.int64) << 32 | whole["b"].astype(np.int64)
    assert (np.diff(key) >= 0).all(), "ordered by (a, b)"
    assert [] in case["cuts"], "the uncut walk is one of the cuts"
    for cuts in case["cuts"]:
        assert np.array_equal(_whole(case, cuts), whole), cuts


def test_the_table_names_every_seam():
    names = {c["name"] for c in CASES}
    for want in ("disc_at_bit_0", "disc_at_bit_63", "disc_last_of_chunk", "opens_in_bit_63_closes_in_bit_0", "run_across_three_chunks", "neut_chunk_between_conc_chunks",
                 "chrom_change_at_a_chunks_first_record", "chrom_change_on_a_neut_record", "chrom_change_on_a_disc_record", "min_records_exact_and_one_less",
                 "min_bp_exact_and_one_less", "equal_pos_length_0", "multi_allelic_and_out_of_range_are_neut", "haploid", "gq_mask_both_sides", "open_run_at_flush"):
        assert want in names
    assert {"n_vars_%d" % n for n in (0, 1, 63, 64, 65, 129)} <= names and {"samples_%d" % s for s in (2, 64, 65, 130)} <= names


def test_thresholds_filter_in_the_model():
    c = next(c for c in CASES if c["name"] == "min_records_exact_and_one_less")
    m = IbdModel(2, c["min_records"], c["min_bp"])
    ibd_segments(c["D"], c["chrom"], c["pos"], 2, 0, 0, model=m)
    assert m.filtered == {"min_records": 1, "min_bp": 0}
    c = next(c for c in CASES if c["name"] == "min_bp_exact_and_one_less")
    m = IbdModel(2, c["min_records"], c["min_bp"])
    ibd_segments(c["D"], c["chrom"], c["pos"], 2, 0, 0, model=m)
    assert m.filtered == {"min_records": 0, "min_bp": 1}


def test_no_flush_keeps_the_open_run():
    c = next(c for c in CASES if c["name"] == "open_run_at_flush")
    m = IbdModel(2, 1, 0)
    assert len(m.step(c["D"], c["chrom"], c["pos"], flush=False)) == 0 and m.open.all()
    assert len(m.step(c["D"][:0], c["chrom"][:0], c["pos"][:0], flush=True)) == 1 and not m.open.any()


def test_planes_from_words_is_the_bit_transpose():
    rng = np.random.default_rng(3)
    words = rng.integers(0, 1 << 63, size=(2, 3, 70), dtype=np.uint64)
    planes = planes_from_words(words)
    assert planes.shape == (128, 3, 2)
    for g, d, v, p in ((0, 0, 0, 0), (1, 2, 69, 63), (0, 1, 63, 5), (1, 0, 64, 62)):
        assert int(planes[64 * g + p, d, v >> 6]) >> (v & 63) & 1 == int(words[g, d, v]) >> p & 1
    assert not (planes[:, :, 1] >> np.uint64(6)).any(), "bits at and beyond n_vars are 0"


@pytest.mark.parametrize("n_samples,n_vars,min_records,seed", ibd_cases.RANDOM)
def test_a_random_case_emits_and_filters(n_samples, n_vars, min_records, seed):
    c = ibd_cases.random_case(n_samples, n_vars, min_records, seed)
    m = IbdModel(n_samples, min_records, c["min_bp"])
    whole = ibd_segments(c["D"], c["chrom"], c["pos"], n_samples, 0, 0, model=m)
    assert len(whole) >= 1 and m.filtered["min_bp"] >= 1
    assert m.filtered["min_records"] >= 1 or min_records == 1            # (n >= 1 holds for every run: min_records 1 cannot filter)
    assert len(np.unique(c["chrom"])) == 3
    if n_samples <= 17:                                                 # the cuts, where the model is quick
        for cuts in c["cuts"][1:]:
            assert np.array_equal(_whole(c, cuts), whole)


# ---- the seam cases ---------------------------------------------------------------------------------------------------------------------

SEAMS = ibd_cases.seam_cases()


@pytest.mark.parametrize("case", SEAMS, ids=[c["name"] for c in SEAMS])
def test_a_seam_case_hits_its_seam_and_does_not_depend_on_the_cuts(case):
    test_a_directed_case_hits_its_seam_and_does_not_depend_on_the_cuts(case)
    whole = _whole(case)
    if "only" in case:                                                   # one pair has segments; every other pair none, in the model
        assert len(whole) == 3 and {(int(s["a"]), int(s["b"])) for s in whole} == {case["only"]}
        assert (case["D"][:, [s for s in range(case["n_samples"]) if s not in case["only"]]] == -1).all()
    if any(s.startswith("all_pairs_") for s in case["seams"]):
        S = case["n_samples"]
        per_pair = np.bincount(whole["a"].astype(np.int64) * S + whole["b"], minlength=S * S).reshape(S, S)[np.triu_indices(S, 1)]
        assert per_pair.min() >= 1 and len(set(per_pair.tolist())) >= 8, "every pair has segments, and the counts differ"


def test_the_seam_cases_claim_every_seam():
    assert set().union(*(c["seams"] for c in SEAMS)) == ibd_cases.IBD_SEAMS
    assert ibd_cases.CHUNK_RECORDS == 2048 and {len(c["D"]) for c in SEAMS if any(s.startswith("step_") for s in c["seams"])} == {2048, 2049, 4096, 4097}
    for S in (15, 16, 17, 31, 32, 33):
        pairs = {c["only"] for c in SEAMS if "only" in c and c["n_samples"] == S}
        assert pairs == {p for p in ((0, 15), (15, 16), (0, 16), (16, 17)) if p[1] < S} | {(S - 2, S - 1)}
    # a cut at the seam is among every chunk case's cuts, and so is the uncut walk: the second trip through the chunk loop
    for c in SEAMS:
        if any(s.startswith("step_") for s in c["seams"]):
            assert [] in c["cuts"] and any(ibd_cases.CHUNK_RECORDS in cut for cut in c["cuts"])


def test_the_start_word_decoy_is_the_other_case_one_trip_off():
    """a change at record 69 alone and at record 2,048 + 69 alone: bit 5 of start word 1 and of start word 33 -- what a walk that stages the
    first trip's start words again would confuse"""
    by = {c["name"]: c for c in SEAMS}
    a, b = by["chrom_change_inside_the_first_trip_alone"], by["chrom_change_inside_the_second_trip_alone"]
    ca, cb = (int(np.flatnonzero(np.diff(c["chrom"]))[0]) + 1 for c in (a, b))
    assert (ca, cb) == (69, 2048 + 69) and (ca >> 6) + ibd_cases.PAIR_CHUNK == cb >> 6 and ca & 63 == cb & 63 == 5
    assert len(_whole(a)) == len(_whole(b)) == 2 and _kind_all(a, 2048 + 69) and _kind_all(b, 69)


def _kind_all(c, v):
    return ibd_cases._kind(c, v) == "CONC" and c["chrom"][v] == c["chrom"][v - 1]


@pytest.mark.parametrize("sample", ibd_cases.TR_SAMPLES)
def test_a_transpose_case_is_the_bit_transpose(sample):
    for record in ibd_cases.TR_RECORDS:
        words, planes = ibd_cases.transpose_case(sample, record)
        assert np.array_equal(planes_from_words(words), planes)
        assert sum(bin(int(x)).count("1") for x in planes.reshape(-1)) == 2
        alone = ibd_cases.transpose_case(sample, record, decoy=False)[1]
        assert sum(bin(int(x)).count("1") for x in alone.reshape(-1)) == 1 and int(alone[sample, (sample + record) % 3, record >> 6]) == 1 << (record & 63)
    assert set(ibd_cases.TR_RECORDS) == {0, 63, 64, 255, 256, 1023, 1024, ibd_cases.TR_N - 1} and ibd_cases.IBD_TR_WORDS * 64 == 1024
