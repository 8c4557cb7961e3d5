"""The record loop on the device (mg_cover_blocks, mg_index_blocks: csrc/block_pipeline.h, csrc/variant_kernels.h) on the directed
panels of tests/block_cases.py: every fixed capacity that decides a record's tier, exactly on it, one below and one above.

Index and reference come from the C oracle (pinned to the Python model on these very panels by tests/test_block_cases_cpu.py),
every key with a 16-bit counter of its own.  What is asserted is exact: the overflow flags equal the restated dealing rules'
prediction record by record -- set on the designated over-capacity records and nowhere else --, EVERY other record's coverage
equals the oracle's, the numbers of records tier 1 listed and tier 3 took equal the prediction, and the chain kernel hands chains to the list path
exactly on the far side of its own limits."""
import functools

import numpy as np
import pytest

import block_cases as bc
from malva_amd import BF_ALT, BF_CTX, Context
from malva_amd.capi import rows_of
from oracle import capi as ocapi

pytestmark = pytest.mark.gpu

BITS = 1 << 24
ACGT = set(b"ACGT")


@functools.lru_cache(maxsize=None)
def _setup(name):
    case = bc.get(name)
    args = case.args()
    obf, omap = bc.oracle_index(case, args, BITS)
    want = ocapi.cover_blocks(obf, omap, case.reference, **args, haploid=case.haploid, k=case.k)
    return case, args, obf, omap, want


def _context(case):
    ctx = Context(case.k, min(case.k + 8, 64), BITS)
    for opt, value in case.options:
        ctx.set_option(opt, value)
    ctx.reference_upload(case.reference)
    return ctx


def _runs(name):
    """(options, sparse) of every run of a case: default, without the chain kernel; the panel-width and tier-1 classes also without
    fw_snp_kernel and with the genotypes handed over sparse"""
    runs = [({}, False), ({"use_chain_kernel": 0}, False)]
    if name[0] in "AE":
        runs += [({"use_snp_kernel": 0}, False), ({}, True)]
    return runs


@pytest.mark.parametrize("name", list(bc.CASES))
def test_cover_blocks_at_the_capacity(name):
    case, args, obf, omap, want = _setup(name)
    deal = bc.deal(case)
    want_ovf = np.array([d["tier"] == "host" for d in deal], dtype=np.uint8)
    want_tier3 = sum(d["took3"] for d in deal)
    want_general = sum(d["tier"] != "lone" for d in deal)      # what tier 1 does not take itself it lists
    slots = np.diff(np.array(args["var_allele_off"]))
    kept = np.repeat(want_ovf == 0, slots)
    assert (want[kept] > 0).sum() > 2000
    items = [(k_, v_) for k_, v_ in omap.items() if set(k_) <= ACGT]
    with _context(case) as ctx:
        ctx.bf_import_sparse(BF_ALT, 1, BITS, obf.set_positions(), obf.counts())
        ctx.bf_import_sparse(BF_CTX, 1, BITS, np.zeros(0, np.uint64), np.zeros(0, np.uint16))
        ctx.map_import([k_ for k_, _ in items], np.array([v for _, v in items], dtype=np.int32))
        for opts, sparse in _runs(name):
            for opt in ("use_chain_kernel", "use_snp_kernel"):
                ctx.set_option(opt, opts.get(opt, 1))
            cov, ovf = ctx.cover_blocks(**args, haploid=case.haploid, sparse=sparse)
            general, tier3 = ctx.blocks_stats()[3], ctx.blocks_stats()[6]
            listed = ctx.get_option("blocks_listed_chains")
            print("%s %s sparse=%d: flagged %d (predicted %d), tier 3 took %d (predicted %d), listed chains %d"
                  % (name, opts, sparse, int(ovf.sum()), int(want_ovf.sum()), tier3, want_tier3, listed))
            assert np.array_equal(ovf, want_ovf), "flagged %s, predicted %s" % (np.flatnonzero(ovf)[:20], np.flatnonzero(want_ovf)[:20])
            assert np.array_equal(cov[kept], want[kept]), "first differing slot %d" % np.flatnonzero(cov[kept] != want[kept])[0]
            assert not cov[~kept].any()
            assert general == want_general, "tier 1 listed %d records, predicted %d" % (general, want_general)
            if case.exact_tier3:
                assert tier3 == want_tier3
            else:
                assert tier3 > 0
            if "listed" in case.claim and opts.get("use_chain_kernel", 1):
                assert (listed > 0) == case.claim["listed"]


@pytest.mark.parametrize("name", [n for n in bc.CASES if n[0] in "ABCE"])
def test_index_blocks_at_the_capacity(name):
    """what mg_index_blocks hands back goes through the model and the batch calls, as the CLI's host enumerator does: the `bf` bits
    and the exact map's keys equal the oracle's index, and the flags equal the prediction (the counting pass and the insert
    pass route every record the same way, or keys would be missing or rows left over)"""
    case, args, obf, omap, _ = _setup(name)
    deal = bc.deal(case, index=True)
    want_ovf = np.array([d["tier"] == "host" for d in deal], dtype=np.uint8)
    with _context(case) as ctx:
        ovf = ctx.index_blocks(**args, haploid=case.haploid)
        print("%s: flagged %d (predicted %d)" % (name, int(ovf.sum()), int(want_ovf.sum())))
        assert np.array_equal(ovf, want_ovf), "flagged %s, predicted %s" % (np.flatnonzero(ovf)[:20], np.flatnonzero(want_ovf)[:20])
        ref_rows, alt_rows = [], []
        bo = args["blk_var_off"]
        for b, (vb, contig) in enumerate(case.blocks):
            if not ovf[bo[b]:bo[b + 1]].any():
                continue
            for per in vb.extract_kmers(case.refs[contig], case.haploid).values():
                for a, sigs in per.items():
                    for sig in sigs:
                        (ref_rows if a == 0 else alt_rows).extend(km.encode() for km in sig)
        if ref_rows:
            ctx.map_insert(rows_of(ref_rows, 136))
        if alt_rows:
            ctx.bf_insert(BF_ALT, rows_of(alt_rows, 136))
        ctx.bf_finalize(BF_ALT)
        assert np.array_equal(ctx.bf_export_sparse(BF_ALT)[2], obf.set_positions())
        keys, vals = ctx.map_export()
        assert sorted(keys) == sorted(k_ for k_, _ in omap.items()) and len(keys) > 20 and not vals.any()
        assert ctx.map_size() == len(keys) == len(set(keys))
