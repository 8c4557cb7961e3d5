"""The gate sized in words (options gate_words / gate_resident_kib; BFView::gate_words): set and test go through the same
inline functions, so every form that reads the gate -- the SoA and compact filter kernels, the scan without summaries, inserts
before and after finalize, the reads path -- must leave the oracle's counters.  A gate that closes on a true entry shows up as
a missing count.  The word mapping itself is checked without a GPU in test_gate_span_cpu.py."""
import functools

import numpy as np
import pytest

from gpu_util import build_index_pair, map_values_by_key, pad_rows
from malva_amd import BF_ALT, BF_CTX, Context, synth
from oracle import capi as ocapi
from test_gpu_reads import random_reads
from test_gpu_scan import _scan_case

pytestmark = pytest.mark.gpu

# (k, ref_k, filter bits, table rows): a full-size filter, a tiny one (collisions, context hits), an odd modulus
CASES = [(35, 43, 1 << 33, 120000), (35, 43, 1 << 17, 150003), (31, 41, (1 << 18) + 77, 100000)]
WORDS = [3, 24, 40]


def _direct_sized(words):
    def check(ctx):
        assert ctx.get_option("gate_words") == words
        assert ctx.get_option("pregate_k") == 0
        assert ctx.get_option("scan_bins") == ctx.get_option("scan_tickets") == ctx.get_option("scan_subs") == 0
    return check


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("k,ref_k,bits,n_rows", CASES)
def test_scan_soa_rows_with_a_sized_gate(k, ref_k, bits, n_rows, words):
    obf, octx, n_hits = _scan_case(k, ref_k, bits, 3000, n_rows, 310, options=[("gate_words", words)], after=_direct_sized(words))
    assert obf.counts().any() and n_hits > 0


@functools.lru_cache(maxsize=None)
def _compact_reference(k, ref_k, bits, n_rows):
    """the oracle's counters after one scan of the table, computed once per shape and left unchanged"""
    panel = synth.snp_panel(3000, 70 + k)
    hi, lo, cnt = synth.kmer_table(panel, n_rows, k, ref_k, 71)
    cnt[:] = 1 + (cnt * 37) % ((1 << (96 - 2 * ref_k)) - 1)
    obf, octx, omap = ocapi.BF(bits), ocapi.BF(bits), ocapi.KMAP()
    sig_rows, valid = synth.signature_rows(panel, k)
    is_ref = np.zeros(sig_rows.shape[0], dtype=np.uint8)
    is_ref[panel.var_allele_off[:-1]] = 1
    ocapi.add_kmers(obf, omap, pad_rows(sig_rows[valid]), is_ref[valid])
    obf.switch_mode()
    ocapi.ref_scan(obf, octx, panel.genome.tobytes(), k, ref_k)
    octx.switch_mode()
    ocapi.kmc_scan_packed(octx, obf, omap, hi, lo, cnt, k, ref_k)
    counts = obf.counts().copy()
    counts.setflags(write=False)
    return panel, (hi, lo, cnt), counts, dict(omap.items())


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("k,ref_k,bits,n_rows", CASES)
def test_scan_compact_rows_with_a_sized_gate(k, ref_k, bits, n_rows, words):
    import torch
    panel, (hi, lo, cnt), want_counts, want_map = _compact_reference(k, ref_k, bits, n_rows)
    with Context(k, ref_k, bits) as ctx:
        ctx.set_option("gate_words", words)
        build_index_pair(ctx, panel, k, ref_k, bits)
        dev = torch.device("cuda", 0)
        d_hi, d_lo = (torch.from_numpy(a.view(np.int64)).to(dev) for a in (hi, lo))
        d_cnt = torch.from_numpy(cnt.view(np.int32)).to(dev)
        d_rows = torch.zeros(ctx.kmc_rows_bytes(n_rows) // 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.kmc_pack_rows_device(d_hi.data_ptr(), d_lo.data_ptr(), d_cnt.data_ptr(), n_rows, d_rows.data_ptr())
        ctx.kmc_scan_rows_device(d_rows.data_ptr(), n_rows)
        ctx.synchronize()
        assert want_counts.any()
        assert np.array_equal(ctx.bf_export(BF_ALT)[3], want_counts)
        assert map_values_by_key(ctx) == want_map
        _direct_sized(words)(ctx)


def test_scan_without_summaries_is_identical_with_a_sized_gate():
    _scan_case(35, 43, 1 << 17, 2000, 80000, 13, use_summary=0, options=[("gate_words", 24)])
    _scan_case(35, 43, 1 << 17, 2000, 80000, 13, use_summary=1, options=[("gate_words", 24)], after=_direct_sized(24))


@pytest.mark.parametrize("words", [3, 40])
def test_keys_inserted_before_and_after_finalize(words):
    """half of the exact map's keys arrive after mg_bf_finalize has sized and rebuilt the gate: gate_set on the sized gate"""
    k, ref_k, bits = 35, 43, 1 << 20
    panel = synth.snp_panel(3000, 55)
    sig_rows, valid = synth.signature_rows(panel, k)
    is_ref = np.zeros(sig_rows.shape[0], dtype=np.uint8)
    is_ref[panel.var_allele_off[:-1]] = 1
    rows, isr = pad_rows(sig_rows[valid]), is_ref[valid]
    obf, octx, omap = ocapi.BF(bits), ocapi.BF(bits), ocapi.KMAP()
    ocapi.add_kmers(obf, omap, rows, isr)
    obf.switch_mode()
    ocapi.ref_scan(obf, octx, panel.genome.tobytes(), k, ref_k)
    octx.switch_mode()
    hi, lo, cnt = synth.kmer_table(panel, 100000, k, ref_k, 56)
    ocapi.kmc_scan_packed(octx, obf, omap, hi, lo, cnt, k, ref_k)
    keys = rows[isr == 1]
    with Context(k, ref_k, bits) as ctx:
        ctx.set_option("gate_words", words)
        ctx.map_insert(keys[0::2])
        ctx.bf_insert(BF_ALT, rows[isr == 0])
        ctx.bf_finalize(BF_ALT)
        assert ctx.get_option("gate_words") == words
        ctx.map_insert(keys[1::2])
        ctx.ref_scan(panel.genome.tobytes())
        ctx.bf_finalize(BF_CTX)
        ctx.kmc_scan(hi, lo, cnt)
        assert ctx.get_option("gate_words") == words
        assert np.array_equal(ctx.bf_export(BF_ALT)[3], obf.counts())
        got, want = map_values_by_key(ctx), dict(omap.items())
        assert got == want and sum(1 for v in want.values() if v) > 1000


def test_reads_path_with_a_sized_gate():
    """row_gate_open on a 24-word gate: the counters the reads leave equal those on the same index with the default gate"""
    k, ref_k, bits = 35, 43, 1 << 22
    panel = synth.snp_panel(3000, seed=5)
    reads = random_reads(panel.genome, panel, np.random.default_rng(8), 3000)   # (ALT bases at half of the sites, both strands)
    fasta = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads))
    seqs = b"\n".join(line for line in fasta.split(b"\n") if not line.startswith(b">")) + b"\n"
    res = []
    for words in (0, 24):
        with Context(k, ref_k, bits, device=0) as ctx:
            if words:
                ctx.set_option("gate_words", words)
            build_index_pair(ctx, panel, k, ref_k, bits)
            assert ctx.get_option("gate_words") == words
            ctx.reads_begin(1, 255)
            ctx.reads_add(seqs)
            n_kept = ctx.reads_finish()
            res.append((n_kept, ctx.bf_export(BF_ALT)[3].copy(), ctx.bf_export(BF_CTX)[3].copy(), map_values_by_key(ctx)))
    (n0, a0, c0, m0), (n1, a1, c1, m1) = res
    assert n0 > 0 and a0.any() and any(m0.values())
    assert np.array_equal(a0, a1) and np.array_equal(c0, c1) and m0 == m1


def test_resident_option_sizes_an_l2_sized_gate_only():
    """the sizing rule lands on 2^25 bits for a small index in a full-size filter: gate_resident_kib replaces that gate and no
    other.  gate_log2 still reports 25 (at most 2^gate_log2 bits).

    The sized gate must also FILTER (a gate that lets every row through leaves the oracle's counters too).  About 6,000 entries of
    4 bits each: in the 3 MiB gate and in the 4 MiB one a word holds an entry with probability 0.015 and a foreign row then needs
    its 4 positions among that entry's 4 of 64 -- 2e-7 per row, 0.02 rows of the table's 100,000.  Both gates therefore let through
    the rows that share a slot with an entry and, but for a handful, nothing else: the two counts differ by at most 5.  A gate of
    2,048 words holds 2.9 entries a word (Poisson); a word with n entries has 1 - exp(-n / 16) of its bits set, a foreign row
    passes with that to the 4th power: 1e-3 at n = 3, 1e-2 at n = 6, 3e-3 on average -- bounded here by 2 rows in 100."""
    n_rows = 100000
    opened = {}

    def sized(ctx):
        assert ctx.get_option("gate_words") == 3072 * 128 and ctx.get_option("gate_log2") == 25
        _direct_sized(3072 * 128)(ctx)
        opened["resident"] = ctx.scan_stats()[3]
    _scan_case(35, 43, 1 << 33, 3000, n_rows, 71, options=[("gate_resident_kib", 3072)], after=sized)

    def off(ctx):
        assert ctx.get_option("gate_words") == 0 and ctx.get_option("gate_log2") == 25
        opened["power of two"] = ctx.scan_stats()[3]
    _scan_case(35, 43, 1 << 33, 3000, n_rows, 71, options=[("gate_resident_kib", 0)], after=off)

    def narrow(ctx):
        _direct_sized(2048)(ctx)
        opened["2048 words"] = ctx.scan_stats()[3]
    _scan_case(35, 43, 1 << 33, 3000, n_rows, 71, options=[("gate_words", 2048)], after=narrow)
    print("rows through the gate:", opened)
    assert 0 < opened["power of two"] < n_rows // 2
    assert abs(opened["resident"] - opened["power of two"]) <= 5
    assert opened["power of two"] - 5 <= opened["2048 words"] <= opened["power of two"] + n_rows // 50

    def small(ctx):
        assert ctx.get_option("gate_words") == 0 and ctx.get_option("gate_log2") == 17
    _scan_case(35, 43, 1 << 17, 3000, n_rows, 71, options=[("gate_resident_kib", 3072)], after=small)


def test_sliced_forms_of_an_l2_sized_gate_keep_the_power_of_two():
    """gate_log2 unset, so the sizing rule lands on 2^25 bits and would size the gate -- but the sub-slice or the ticket form takes
    gates of that size here (their thresholds lowered): they cut the gate by word index, and it stays a power of two"""
    def subs(ctx):
        assert ctx.get_option("gate_log2") == 25 and ctx.get_option("gate_words") == 0
        assert ctx.get_option("scan_subs") == 32 and ctx.get_option("scan_tickets") == 0      # 2^19 words in pieces of 2^14
    _scan_case(35, 43, 1 << 33, 3000, 150000, 31, after=subs, options=[("gate_resident_kib", 3072), ("use_sub", 1), ("sub_min_log2", 11)])
    _scan_case(35, 43, 1 << 33, 3000, 150000, 31, after=subs, options=[("gate_words", 40), ("use_sub", 1), ("sub_min_log2", 11)])

    def tickets(ctx):
        assert ctx.get_option("gate_log2") == 25 and ctx.get_option("gate_words") == 0
        assert ctx.get_option("scan_tickets") == 2 and ctx.get_option("scan_subs") == 0       # 2^19 words in slices of 2^18
    _scan_case(35, 43, 1 << 33, 3000, 150000, 31, after=tickets,
               options=[("gate_resident_kib", 3072), ("use_sub", 0), ("use_tickets", 1), ("ticket_min_log2", 11)])


def test_a_sized_gate_is_never_cut_into_slices():
    """the thresholds of the sliced forms lowered AFTER finalize has made a sized gate: the scan stays with the direct form
    (scan_plan), whose kernels are the ones that know the sized gate's word index"""
    k, ref_k, bits = 35, 43, 1 << 20
    panel = synth.snp_panel(3000, 55)
    hi, lo, cnt = synth.kmer_table(panel, 100000, k, ref_k, 56)
    with Context(k, ref_k, bits) as ctx:
        ctx.set_option("gate_words", 40)
        obf, octx, omap = build_index_pair(ctx, panel, k, ref_k, bits)
        ocapi.kmc_scan_packed(octx, obf, omap, hi, lo, cnt, k, ref_k)
        assert ctx.get_option("gate_words") == 40
        for name, value in [("use_sub", 1), ("sub_min_log2", 5), ("sub_words_log2", 3), ("use_tickets", 1), ("ticket_min_log2", 5)]:
            ctx.set_option(name, value)
        ctx.kmc_scan(hi, lo, cnt)
        _direct_sized(40)(ctx)
        assert np.array_equal(ctx.bf_export(BF_ALT)[3], obf.counts())
        assert map_values_by_key(ctx) == dict(omap.items())


def test_ticket_and_sub_slice_forms_ignore_the_resident_option():
    def tickets(ctx):
        assert ctx.get_option("gate_words") == 0 and ctx.get_option("scan_tickets") >= 2 and ctx.get_option("scan_subs") == 0
    _scan_case(35, 43, 1 << 33, 3000, 150000, 31, after=tickets,
               options=[("gate_resident_kib", 3072), ("pregate_log2", 10), ("gate_log2", 14), ("use_tickets", 1), ("ticket_min_log2", 11)])

    def subs(ctx):
        assert ctx.get_option("gate_words") == 0 and ctx.get_option("scan_subs") >= 2 and ctx.get_option("scan_tickets") == 0
    _scan_case(35, 43, 1 << 33, 3000, 150000, 31, after=subs,
               options=[("gate_resident_kib", 3072), ("gate_log2", 14), ("use_sub", 1), ("sub_min_log2", 11), ("sub_words_log2", 3)])
