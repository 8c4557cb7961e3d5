"""mg_blocks_host as the binding lays it out (capi.BlocksHost) against the library's, and the host forms' own argument checks.

One hand-made panel sets every member at once, with arrays that differ in content wherever two members have the same type, so that a member
at the wrong offset or two swapped pointers give other coverages: three blocks on two contigs behind 64 bases of padding (two distinct
non-zero blk_ref_base, two distinct blk_ref_len), a lone SNP (tier 1), chains, a record of three alleles with an indel (ref_size != min_size),
a repeated ALT text (canon is not the identity), a record that is not present, three samples with phased and unphased genotypes.  Index and
coverages come from the C oracle, every key with a counter of its own (block_cases.oracle_index).

The CPU half shows on the oracle alone that the panel cares: min_size, present, canon, the two blk_ref_base and the default word of the sparse
form each change the coverages (or the index) when replaced by their neutral value.  The argument table goes through Context's two methods,
whose Python signatures are older than the struct; every row returns before a kernel is launched."""
import contextlib
import ctypes as C
import functools
import re
import types

import numpy as np
import pytest

import block_cases as bc
from block_util import pack_blocks
from malva_amd import BF_ALT, BF_CTX, Context, MalvaError, capi
from oracle import capi as ocapi

gpu = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE = -1, -3
K, REF_K, BITS, PAD = 35, 43, 1 << 20, 64
PHASED0, UNPHASED0 = 1 << 14, 0                  # the two default words of the sparse form: 0|0 and 0/0


@functools.lru_cache(maxsize=None)
def _panel():
    """-> (reference, args, obf, omap, want): the panel's flat arrays, the oracle's index of it and the oracle's coverages"""
    rng = np.random.default_rng(77)
    seq = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)).decode()
    refs = {"1": seq(1500), "2": seq(900)}
    b = bc.Builder("abi", K, n_samples=3, refs=refs)
    r1, r2 = refs["1"], refs["2"]
    other = lambda base: "ACGT"[("ACGT".index(base) + 1) % 4]
    # block 0: a lone SNP
    b.rec("1", 100, gts=[(0, 1), (1, 1), (0, 0)], phasing=[True, False, True])
    # block 1: a chain.  Y is near the indel only through ref_size - min_size = 4 (are_near: 306 + 5 - 1 - 1 + 18 = 327), and allele 2 of the
    # indel occurs only on a haplotype that carries Y's ALT; NP is not present but has genotypes; DUP repeats its ALT text
    b.rec("1", 300, gts=[(1, 0), (0, 1), (1, 1)], phasing=[True, True, False])
    b.rec("1", 306, ref_len=5, alts=[r1[306], r1[306:311] + "GG"], gts=[(1, 0), (2, 0), (0, 1)], phasing=[True, True, True])
    b.rec("1", 327, gts=[(0, 0), (1, 0), (0, 0)], phasing=[True, True, True])
    b.rec("1", 335, gts=[(0, 1), (1, 0), (1, 1)], phasing=[True, True, True], present=False)
    b.rec("1", 340, alts=[other(r1[340])] * 2, gts=[(0, 2), (1, 0), (2, 2)], phasing=[True, True, False])
    # block 2, on the other contig: sample 0 is 0/0 UNPHASED at the first record and heterozygous at the four behind it, so all sixteen picks
    # of those four are signatures -- and only two of them once the first record's word reads 0|0 (a coverage is the best of its signatures:
    # each of the eight alleles keeps its value with probability 1/8)
    b.rec("2", 200, gts=[(0, 0), (1, 0), (0, 1)], phasing=[False, True, False])
    b.rec("2", 206, gts=[(0, 1), (0, 0), (1, 0)], phasing=[True, True, False])
    b.rec("2", 212, gts=[(1, 0), (0, 1), (0, 0)], phasing=[True, True, True])
    b.rec("2", 218, gts=[(0, 1), (0, 0), (0, 0)], phasing=[True, True, True])
    b.rec("2", 224, gts=[(1, 0), (0, 0), (0, 0)], phasing=[True, True, True])
    case = b.finish()
    assert [len(vb.variants) for vb, _ in case.blocks] == [1, 5, 5]
    base, lens = {"1": PAD, "2": PAD + len(r1)}, {n: len(s) for n, s in refs.items()}
    args = pack_blocks(case.blocks, base, lens)
    reference = (seq(PAD) + r1 + r2).encode()
    obf, omap = bc.oracle_index(types.SimpleNamespace(reference=reference, haploid=False, k=K), args, BITS)
    want = ocapi.cover_blocks(obf, omap, reference, **args, haploid=False, k=K)
    return reference, args, obf, omap, want


def _cover(**changed):
    reference, args, obf, omap, _ = _panel()
    return ocapi.cover_blocks(obf, omap, reference, **{**args, **changed}, haploid=False, k=K)


def _index_keys(args):
    obf, omap = ocapi.BF(BITS), ocapi.KMAP()
    ocapi.index_blocks(obf, omap, _panel()[0], **args, haploid=False, k=K)
    obf.switch_mode()
    return obf.set_positions(), sorted(key for key, _ in omap.items())


# ---- the CPU half: the panel cares about every member ---------------------------------------------------------------------------------

def test_the_panel_holds_what_it_claims():
    _, args, _, _, want = _panel()
    a = {key: np.asarray(v) for key, v in args.items()}
    assert len(a["blk_ref_base"]) == 3 and len(set(a["blk_ref_base"])) == 2 and a["blk_ref_base"].min() > 0 and len(set(a["blk_ref_len"])) == 2
    assert (a["ref_size"] != a["min_size"]).any() and (np.diff(a["var_allele_off"]) == 3).any()
    assert (a["canon"] != np.concatenate([np.arange(n) for n in np.diff(a["var_allele_off"])])).any()
    assert (a["present"] == 0).sum() == 1 and args["n_samples"] == 3
    words = a["gt"][a["present"] != 0]
    assert (words == PHASED0).any() and (words == UNPHASED0).any()
    assert ((words & 0x3FFF != 0) & (words >> 14 == 1)).any() and ((words & 0x3FFF != 0) & (words >> 14 == 0)).any()
    slots = np.repeat(a["present"], np.diff(a["var_allele_off"])).astype(bool) & (a["canon"] == np.concatenate([np.arange(n) for n in np.diff(a["var_allele_off"])]))
    assert (want[slots] > 0).all(), "every allele of a present record is covered: %s" % want
    assert len(set(want[slots])) > len(want[slots]) // 2, "the counters tell the keys apart"


@pytest.mark.parametrize("member", ["min_size", "present", "canon", "blk_ref_base"])
def test_a_neutral_member_changes_the_coverages(member):
    _, args, _, _, want = _panel()
    neutral = {"min_size": args["ref_size"], "present": np.ones(len(args["pos"]), np.uint8),
               "canon": np.concatenate([np.arange(n) for n in np.diff(args["var_allele_off"])]),
               "blk_ref_base": [{PAD: PAD + 1500, PAD + 1500: PAD}[x] for x in args["blk_ref_base"]]}[member]
    assert not np.array_equal(np.asarray(neutral), np.asarray(args[member]))
    try:
        got = _cover(**{member: neutral})
    except IndexError:                                     # (rejected: the reference throws)
        return
    assert not np.array_equal(got, want), member


def test_the_default_word_of_the_sparse_form_matters():
    """entries made against one default word and read with the other: 0/0 read as 0|0 takes signatures away (other coverages), 0|0 read as
    0/0 adds signatures (other keys in the index)"""
    _, args, _, _, want = _panel()
    gt = np.asarray(args["gt"])
    as_phased = np.where(gt == UNPHASED0, PHASED0, gt).astype(np.uint16)
    as_unphased = np.where(gt == PHASED0, UNPHASED0, gt).astype(np.uint16)
    assert not np.array_equal(_cover(gt=as_phased), want)
    bits, keys = _index_keys(args)
    more_bits, more_keys = _index_keys({**args, "gt": as_unphased})
    assert len(more_bits) > len(bits) or len(more_keys) > len(keys)


# ---- the GPU half ---------------------------------------------------------------------------------------------------------------------

def _import_index(ctx, obf, omap):
    ctx.bf_import_sparse(BF_ALT, 1, BITS, obf.set_positions(), obf.counts())
    ctx.bf_import_sparse(BF_CTX, 1, BITS, np.zeros(0, np.uint64), np.zeros(0, np.uint16))
    items = list(omap.items())
    ctx.map_import([key for key, _ in items], np.array([v for _, v in items], dtype=np.int32))


@pytest.fixture(scope="module")
def covering():
    """a context that holds the panel's reference and the oracle's index, finalised: what mg_cover_blocks needs"""
    reference, _, obf, omap, _ = _panel()
    with Context(K, REF_K, BITS) as ctx:
        ctx.reference_upload(reference)
        _import_index(ctx, obf, omap)
        yield ctx


@pytest.fixture(scope="module")
def indexing():
    """a context that holds the reference alone, before mg_bf_finalize: what mg_index_blocks needs (no test here lets it insert anything)"""
    with Context(K, REF_K, BITS) as ctx:
        ctx.reference_upload(_panel()[0])
        yield ctx


@contextlib.contextmanager
def _two_planes(ctx):
    """cohort mode with the context's own counters in plane 0 and another value for every counter in plane 1, plane 1 selected; the
    context's counters are put back behind mg_cohort_end, which hands the single-sample vectors back zeroed"""
    import torch
    n_bf, n_map = ctx.counters_size()
    first = torch.zeros(n_bf + n_map, dtype=torch.int32, device="cuda:0")
    ctx.counters_export_device(first.data_ptr())
    ctx.synchronize()
    assert bool((first > 0).any())
    second = torch.where(first > 0, (first * 3 + 11) % 60000 + 1, first)
    ctx.cohort_begin(2)
    try:
        for s, t in enumerate((first, second)):
            ctx.cohort_select(s)
            ctx.counters_import_device(t.data_ptr())
        yield
    finally:
        ctx.cohort_end()
        ctx.counters_import_device(first.data_ptr())
        ctx.synchronize()


FORMS = [(False, PHASED0), (True, PHASED0), (True, UNPHASED0)]
FORM_IDS = ["dense", "sparse-0|0", "sparse-0/0"]


@gpu
@pytest.mark.parametrize("sparse,sp_default", FORMS, ids=FORM_IDS)
def test_cover_every_member_at_once(covering, sparse, sp_default):
    _, args, _, _, want = _panel()
    cov, ovf = covering.cover_blocks(**args, haploid=False, sparse=sparse, sp_default=sp_default)
    print("coverages %s, the oracle's %s, flagged %s" % (cov, want, ovf))
    assert not ovf.any()
    assert np.array_equal(cov, want), "first differing slot %d" % np.flatnonzero(cov != want)[0]


@gpu
@pytest.mark.parametrize("sparse,sp_default", FORMS, ids=FORM_IDS)
def test_index_every_member_at_once(sparse, sp_default):
    reference, args, obf, omap, _ = _panel()
    with Context(K, REF_K, BITS) as ctx:
        ctx.reference_upload(reference)
        ovf = ctx.index_blocks(**args, haploid=False, sparse=sparse, sp_default=sp_default)
        assert not ovf.any()
        ctx.bf_finalize(BF_ALT)
        assert np.array_equal(ctx.bf_export_sparse(BF_ALT)[2], obf.set_positions())
        keys, vals = ctx.map_export()
        assert sorted(keys) == sorted(key for key, _ in omap.items()) and len(keys) == len(set(keys)) > 8 and not vals.any()


@gpu
@pytest.mark.parametrize("sparse,sp_default", FORMS, ids=FORM_IDS)
def test_cover_all_planes(covering, sparse, sp_default):
    """two planes with different counters (the oracle's, and another value for every counter): row s of the cohort form is the single-sample
    form with plane s selected, and plane 0's is the oracle's"""
    ctx = covering
    _, args, _, _, want = _panel()
    with _two_planes(ctx):
        planes, ovf = ctx.cover_blocks(**args, haploid=False, sparse=sparse, sp_default=sp_default, all_planes=True)
        assert ctx.cohort_info() == (2, 1)                 # the selected plane is left as it was
        assert planes.shape == (2, len(want)) and not ovf.any()
        assert np.array_equal(planes[0], want) and not np.array_equal(planes[1], want)
        for s in range(2):
            ctx.cohort_select(s)
            cov, ovf = ctx.cover_blocks(**args, haploid=False, sparse=sparse, sp_default=sp_default)
            assert not ovf.any() and np.array_equal(planes[s], cov), "plane %d" % s


# ---- the argument table: every row is a few records and returns before a kernel is launched --------------------------------------------

def _call(ctx, form, args, **kw):
    if form == "cover":
        return ctx.cover_blocks(**args, haploid=False, **kw)
    return ctx.index_blocks(**args, haploid=False, **kw), None


def _fails(ctx, form, args, code, message, **kw):
    with pytest.raises(MalvaError, match=re.escape(message)) as e:
        _call(ctx, form, args, **kw)
    assert e.value.code == code, str(e.value)


def _changed(**changed):
    return {**_panel()[1], **changed}


def _bad_sparse(monkeypatch, how):
    """the sparse triple of the panel, broken in one place (the binding makes the triple itself: capi.sparse_genotypes)"""
    make = capi.sparse_genotypes

    def broken(gt, n_samples, default=PHASED0):
        off, sample, word = make(gt, n_samples, default)
        counts = np.diff(off.astype(np.int64))
        if how == "descend":
            off[0] = off[1] + 1
        elif how == "beyond":
            sample[0] = n_samples
        else:
            v = int(np.flatnonzero(counts >= 2)[0])
            sample[off[v]:off[v] + 2] = sample[off[v]:off[v] + 2][::-1].copy()
        return off, sample, word
    monkeypatch.setattr(capi, "sparse_genotypes", broken)


@gpu
@pytest.mark.parametrize("form", ["cover", "index"])
def test_arrays_that_do_not_fit_are_argument_errors(covering, indexing, monkeypatch, form):
    ctx = covering if form == "cover" else indexing
    args = _panel()[1]
    off = list(args["blk_var_off"])
    _fails(ctx, form, _changed(blk_var_off=off[:-1] + [off[-1] - 1]), MG_ERR_ARG, "block offsets do not close")
    _fails(ctx, form, _changed(pool=args["pool"][:-1]), MG_ERR_ARG, "allele offsets exceed the pool")
    lens = list(args["blk_ref_len"])
    _fails(ctx, form, _changed(blk_ref_len=lens[:-1] + [lens[-1] + 1]), MG_ERR_ARG, "block 2 lies outside the uploaded reference")
    for how, message in (("descend", "sparse genotype offsets of record 0"), ("beyond", "samples must ascend below n_samples"), ("order", "samples must ascend below n_samples")):
        with monkeypatch.context() as m:
            _bad_sparse(m, how)
            _fails(ctx, form, args, MG_ERR_ARG, message, sparse=True)
    _call(ctx, form, _changed(blk_var_off=[0], blk_ref_base=[], blk_ref_len=[], pos=[], ref_size=[], min_size=[], present=[], var_allele_off=[0],
                              allele_off=[0], pool=np.zeros(0, np.uint8), canon=[], gt=np.zeros((0, 3), np.uint16)))   # (no record: nothing to object to)


@gpu
def test_calls_out_of_turn_are_state_errors(covering, indexing):
    args = _panel()[1]
    with Context(K, REF_K, BITS) as fresh:                 # no reference, nothing finalised
        _fails(fresh, "index", args, MG_ERR_STATE, "mg_reference_upload first")
        _fails(fresh, "cover", args, MG_ERR_STATE, "`bf` not finalised")
        fresh.bf_finalize(BF_ALT)
        _fails(fresh, "cover", args, MG_ERR_STATE, "mg_reference_upload first")
        _fails(fresh, "index", args, MG_ERR_STATE, "after mg_bf_finalize")
    _fails(indexing, "cover", args, MG_ERR_STATE, "`bf` not finalised")
    _fails(covering, "index", args, MG_ERR_STATE, "after mg_bf_finalize")
    with _two_planes(covering):                            # (cohort mode needs both filters finalised: the cohort check comes first)
        _fails(covering, "index", args, MG_ERR_STATE, "cohort mode")


@gpu
def test_all_planes_needs_cohort_mode(covering):
    _fails(covering, "cover", _panel()[1], MG_ERR_STATE, "not in cohort mode", all_planes=True)


@gpu
def test_raw_calls(covering, indexing):
    """what no Context method can send: a NULL batch, a batch of records without genotypes in either form, and an empty batch whose outputs
    stay as they are even where nothing else of the call is in order"""
    cov, ovf = (C.c_uint32 * 64)(*[0xAAAAAAAA] * 64), (C.c_uint8 * 64)(*[0xAA] * 64)
    entries = [(covering, lambda ctx, x: ctx._L.mg_cover_blocks(ctx.h, x, 0, cov, ovf)),
               (covering, lambda ctx, x: ctx._L.mg_cover_blocks_cohort(ctx.h, x, 0, cov, ovf)),
               (indexing, lambda ctx, x: ctx._L.mg_index_blocks(ctx.h, x, 0, ovf))]
    for ctx, entry in entries:
        assert entry(ctx, None) == MG_ERR_ARG
    x = capi._blocks_host(**_panel()[1], sparse=False, sp_default=PHASED0)
    x.gt = None
    assert x.n_samples == 3 and not x.sp_off
    with _two_planes(covering):
        for ctx, entry in entries:
            assert entry(ctx, C.byref(x)) == MG_ERR_ARG
        assert entries[1][1](covering, C.byref(capi.BlocksHost())) == 0
    with Context(K, REF_K, BITS) as fresh:
        assert fresh._L.mg_cover_blocks(fresh.h, C.byref(capi.BlocksHost()), 0, cov, ovf) == 0
        assert fresh._L.mg_index_blocks(fresh.h, C.byref(capi.BlocksHost()), 0, ovf) == 0
    assert list(cov) == [0xAAAAAAAA] * 64 and list(ovf) == [0xAA] * 64
