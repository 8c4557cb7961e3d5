"""The call-time k-mer scan on the device against the oracle on the directed cases of tests/scan_cases.py: the direct, ticket,
sub-slice and partition forms at their tile, stage, segment, walk, launch-group and counter seams.  For every case, in order:
the index is built on the device and in the oracle and the filters' bits compared; the table goes through the entry the case
names; every `bf` counter, every exact-map value and the records' copies of the counters (mg_debug_bucket_count) must equal
the oracle's; then the form the scan took, the tickets it spilled, the rows that hit `bf` and the open rows of the last launch
group must be what the restated plan says.  Everything is exact.  tests/test_scan_cases_cpu.py proves, without a GPU, that each
case holds what its name says."""
import numpy as np
import pytest
import torch

import scan_cases as sc
from malva_amd import BF_ALT, BF_CTX, Context
from malva_amd.capi import rows_of

pytestmark = pytest.mark.gpu

LAYOUT = ("gate_log2", "pregate_log2", "map_ordered")           # set before the first insert: part of what a context is
RUNTIME = dict(use_summary=1, scan_rows=2, scan_variant=2, scan_grid=0, probe_grid=0, hits_grid=0, use_hit_entries=1, use_record_counters=1,
               use_tickets=1, ticket_min_log2=28, use_sub=1, sub_min_log2=28, sub_words_log2=14, scan_chunk_log2=27, scan_bin_cap=0,
               ticket_gate_grid=0, sub_grid=0, sub_split=4, lazy_vectors=1, use_pregate=1, use_partition=0, scan_bin_rows=4, scan_bin_ring=0)
FORM_OPTION = {"tickets": "scan_tickets", "subs": "scan_subs", "bins": "scan_bins"}


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def context_of():
    """one context per (setup, layout options, index), shared by the consecutive cases that have it: counters_reset between them"""
    held = {}

    def get(c):
        s = sc.setup(c.setup)
        opts = dict(s.options() + list(c.opts))
        key = (c.setup, tuple((k, opts[k]) for k in LAYOUT if k in opts), None if c.indexed is None else tuple(c.indexed.tolist()))
        if key not in held:
            for ctx in held.values():
                ctx.close()
            held.clear()
            ctx = Context(s.k, s.ref_k, s.bits)
            for name in LAYOUT:
                if name in opts:
                    ctx.set_option(name, opts[name])
            bf, mp, cx, genome = sc.index_of(c)
            if mp:
                ctx.map_insert(rows_of(mp))
            if bf:
                ctx.bf_insert(BF_ALT, rows_of(bf))
            ctx.bf_finalize(BF_ALT)
            if genome is not None:
                ctx.ref_scan(genome)
            if cx:
                ctx.bf_insert(BF_CTX, rows_of(cx))
            ctx.bf_finalize(BF_CTX)
            held[key] = ctx
        return held[key]
    yield get
    for ctx in held.values():
        ctx.close()


def _raw_rows12(s, hi, lo, cnt, pad_row, pad_count):
    """a caller-made compact buffer: three little-endian dwords per row, count << (2 ref_k - 64) above the k-mer's top bits; the
    rows that pad it to a whole quad hold an indexed k-mer with a count"""
    n = len(hi)
    n_pad = (n + 3) // 4 * 4
    hi = np.concatenate([hi, np.full(n_pad - n, s.hi[pad_row], dtype=np.uint64)])
    lo = np.concatenate([lo, np.full(n_pad - n, s.lo[pad_row], dtype=np.uint64)])
    cnt = np.concatenate([cnt, np.full(n_pad - n, pad_count, dtype=np.uint32)]).astype(np.uint64)
    w = np.zeros((n_pad, 3), dtype=np.uint32)
    w[:, 0] = (lo & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    w[:, 1] = (lo >> np.uint64(32)).astype(np.uint32)
    w[:, 2] = (hi | (cnt << np.uint64(2 * s.ref_k - 64))).astype(np.uint32)
    return w


def _scan(ctx, c, s):
    hi, lo, cnt = sc.table(c)
    n = len(hi)
    if c.entry == "host":
        ctx.kmc_scan(hi, lo, cnt)
        return
    dev = torch.device("cuda", 0)
    if c.entry == "rows12-raw":
        d_rows = torch.from_numpy(_raw_rows12(s, hi, lo, cnt, int(c.order[0]), 5).view(np.int32).reshape(-1)).to(dev)
        torch.cuda.synchronize()
        ctx.kmc_scan_rows_device(d_rows.data_ptr(), n)
        ctx.synchronize()
        return
    off = c.offset                                              # the arrays start `off` rows into their allocations
    d_hi = torch.zeros(n + off, dtype=torch.int64, device=dev)
    d_lo = torch.zeros(n + off, dtype=torch.int64, device=dev)
    d_cnt = torch.zeros(n + off, dtype=torch.int32, device=dev)
    d_hi[off:] = torch.from_numpy(hi.view(np.int64)).to(dev)
    d_lo[off:] = torch.from_numpy(lo.view(np.int64)).to(dev)
    d_cnt[off:] = torch.from_numpy(cnt.view(np.int32)).to(dev)
    p_hi, p_lo, p_cnt = d_hi.data_ptr() + 8 * off, d_lo.data_ptr() + 8 * off, d_cnt.data_ptr() + 4 * off
    assert d_hi.data_ptr() % 16 == 0 and d_lo.data_ptr() % 16 == 0 and d_cnt.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    if c.entry == "rows12":
        assert not off
        d_rows = torch.zeros(ctx.kmc_rows_bytes(n) // 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.kmc_pack_rows_device(p_hi, p_lo, p_cnt, n, d_rows.data_ptr())
        ctx.kmc_scan_rows_device(d_rows.data_ptr(), n)
    else:
        ctx.kmc_scan_device(p_hi, p_lo, p_cnt, n)
    ctx.synchronize()                                           # (the tensors live until here)


@pytest.mark.parametrize("name", sc.case_ids())
def test_scan_case(context_of, cus, name):
    c = sc.case(name)
    s = sc.setup(c.setup)
    ctx = context_of(c)
    obf, octx, omap = sc.expected(c)
    m = sc.model(c, obf.words(), cus)
    # index parity first: same bits in both filters
    assert np.array_equal(ctx.bf_export(BF_ALT)[2], obf.words())
    assert np.array_equal(ctx.bf_export(BF_CTX)[2], octx.words())
    opts = dict(RUNTIME)
    opts.update((k, v) for k, v in c.opts if k not in LAYOUT)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.counters_reset()
    _scan(ctx, c, s)
    stats = ctx.scan_stats()[3:]
    # the records' copies as the call-time lookups read them, then the vectors
    pos = obf.set_positions()
    if len(pos):
        rank, count = ctx.bucket_count(pos)
        assert np.array_equal(rank, np.arange(len(pos)))
        bad = np.flatnonzero(count != obf.counts())
        assert bad.size == 0, (bad[:5], count[bad[:5]], obf.counts()[bad[:5]])
    got = ctx.bf_export(BF_ALT)[3]
    bad = np.flatnonzero(got != obf.counts())
    assert bad.size == 0, (bad[:5], got[bad[:5]], obf.counts()[bad[:5]])
    keys, vals = ctx.map_export()
    assert dict(zip(keys, (int(v) for v in vals))) == dict(omap.items())
    if len(pos):                                                # and the copies again, now that the vectors have been asked for
        assert np.array_equal(ctx.bucket_count(pos)[1], obf.counts())
    # the form, and what it reports
    for form, option in FORM_OPTION.items():
        assert ctx.get_option(option) == (m["nbins"] if form == m["form"] else 0), option
    spilled = ctx.get_option("scan_spilled")
    if m["spilled"] is not None:
        assert spilled == m["spilled"], (spilled, m["spilled"])
    elif m["form"] == "bins":                                   # (what spills there depends on the coarse gate: only whether anything does)
        assert (spilled > 0) == bool(c.claims.get("spilled_positive"))
    n_open, n_hits = stats
    assert ctx.scan_stats()[3:] == stats                        # (the exports in between leave the scan's counters alone)
    assert n_hits == m["n_hits"], (n_hits, m["n_hits"])
    assert m["n_open"][0] <= n_open <= m["n_open"][1], (n_open, m["n_open"])


def test_sub_grid_is_clamped_to_what_the_gate_pass_holds():
    """scan_sub_gate_kernel keeps a wave's segment fills one per lane: 64 segments per wave, 1,024 per workgroup (SB_MAXB)"""
    with Context(35, 43, 1 << 20) as ctx:
        for asked, held in ((4096, sc.SB_MAXB), (1025, sc.SB_MAXB), (1024, 1024), (7, 7), (0, 0), (-3, 0)):
            ctx.set_option("sub_grid", asked)
            assert ctx.get_option("sub_grid") == held
