"""Tier 1 of the record loop with every number of tiles a workgroup may take (option lone_tiles: 1, 2, 4, 8, and 0 = by the panel's
size), on panels whose ends sit on, one below and one above a tile (TPB / 2 = 128 records) and the eight tiles of a full
workgroup, and on a mixed panel whose general records are listed from several tiles and workgroups.  Index, scan, cut, cover and
genotype run on the device from a resident panel (tests/test_gpu_resident.py's way); bits, counters, coverages, GT, GQ, overflow
flags and the record loop's counts equal the C oracle's and are the same under every setting.  The cohort kernel and the index
kernel take the same argument: two planes against the single-sample call, and the filter bits and the exact map after an index.
The redo kernel (alleles with a base outside ACGT in their window) walks the same groups of tiles on a grid of its own: one panel
has more groups than that grid.  The cover call's one clear kernel is given flags at an odd address."""
import functools

import numpy as np
import pytest
import torch

import block_cases as bc
from gpu_util import map_values_by_key
from malva_amd import BF_ALT, BF_CTX, Context, MalvaError, synth
from malva_amd.resident import ResidentCohort, ResidentPanel
from oracle import capi as ocapi
from test_gpu_resident import oracle_blocks

pytestmark = pytest.mark.gpu

K, REF_K = 35, 43
SETTINGS = [0, 1, 2, 4, 8]
SEAMS = [1, 127, 128, 129, 1023, 1024, 1025]      # records: a tile is 128, a workgroup of eight tiles 1,024


# ---- the panels ---------------------------------------------------------------------------------------------------------------
def mixed_case():
    """90 clusters of two or three SNPs a few bases apart (blocks of two and three: general records), each followed by ten lone
    SNPs: 1,125 records, general records in every tile of 128 and in both workgroups of eight tiles"""
    b = bc.Builder("lone-tiles-mixed", K, n_samples=8, seed=11)
    for i in range(90):
        base = 3000 + 2000 * i
        for d in (0, 6, 13)[:2 + i % 2]:
            b.rec("1", base + d)
        for j in range(10):
            b.rec("1", base + 300 + 120 * j)
    return b.finish()


def flat_of(case):
    """a block_cases panel as the FlatPanel the resident forms and synth's k-mer tables take: frequencies made up, the donor
    carries what the first sample carries"""
    args = case.args()
    names = case.names
    sizes = np.diff(np.array(args["blk_var_off"], dtype=np.int64))
    vo = np.array(args["var_allele_off"], dtype=np.uint32)
    rng = np.random.default_rng(3)
    freq = np.zeros(int(vo[-1]), dtype=np.float32)
    for v in range(len(vo) - 1):
        f = rng.random(int(vo[v + 1] - vo[v])) + 0.1
        freq[vo[v]:vo[v + 1]] = f / f.sum()
    gt = np.ascontiguousarray(args["gt"], dtype=np.uint16)
    donor = np.stack([gt[:, 0] & 127, (gt[:, 0] >> 7) & 127], axis=1).astype(np.int8)
    return synth.FlatPanel(genome=np.frombuffer(case.reference, dtype=np.uint8).copy(), contig_names=names,
                           contig_base=np.array([case.base[n] for n in names], dtype=np.uint64),
                           contig_len=np.array([len(case.refs[n]) for n in names], dtype=np.uint32),
                           contig_id=np.repeat(np.array([names.index(n) for _, n in case.blocks], dtype=np.uint32), sizes),
                           pos=np.array(args["pos"], dtype=np.int32), ref_size=np.array(args["ref_size"], dtype=np.uint32),
                           min_size=np.array(args["min_size"], dtype=np.uint32), present=np.array(args["present"], dtype=np.uint8), var_allele_off=vo,
                           allele_off=np.array(args["allele_off"], dtype=np.uint32), pool=np.array(args["pool"], dtype=np.uint8),
                           canon=np.array(args["canon"], dtype=np.uint8), freq=freq, gt=gt, n_samples=case.n_samples, donor_gt=donor)


@functools.lru_cache(maxsize=None)
def setup(name):
    """(panel, what the oracle makes of it, (general records, records tier 3 takes) as the dealing rules predict them)"""
    if name == "mixed":
        case = mixed_case()
        panel = flat_of(case)
        deal = bc.deal(case)
        assert not any(d["tier"] == "host" for d in deal)
        want_general, want_tier3 = sum(d["tier"] != "lone" for d in deal), sum(d["took3"] for d in deal)
        listed = np.flatnonzero([d["tier"] != "lone" for d in deal])
        assert want_general >= 200 and len(set(listed // 128)) == 9 and len(set(listed // 1024)) == 2 and panel.n == 1125
        bits, n_rows = 1 << 22, 60_000
    else:
        n = int(name)
        panel = synth.flat_from_snp_panel(synth.snp_panel(n, seed=300 + n))
        want_general, want_tier3 = 0, 0            # 100 nt apart, 1,000 nt from either end: every record is a block, flanks inside
        bits, n_rows = 1 << 22, 20_000 + 20 * n
    args = oracle_blocks(panel, K)
    obf, octx, omap = ocapi.BF(bits), ocapi.BF(bits), ocapi.KMAP()
    ocapi.index_blocks(obf, omap, panel.genome, **args, haploid=False, k=K)
    obf.switch_mode()
    for b, l in zip(panel.contig_base, panel.contig_len):
        ocapi.ref_scan(obf, octx, panel.genome[int(b):int(b) + int(l)].tobytes(), K, REF_K)
    octx.switch_mode()
    table = synth.flat_kmer_table(panel, n_rows, K, REF_K, seed=7)
    ocapi.kmc_scan_packed(octx, obf, omap, *table, K, REF_K)
    stats = {}
    cov = ocapi.cover_blocks(obf, omap, panel.genome, **args, haploid=False, k=K, stats=stats)
    g1, g2, gq = ocapi.genotype_panel(cov, panel.freq, panel.var_allele_off, 0.001, 200, False)
    assert (cov > 0).sum() >= max(1, panel.n // 4)
    want = dict(args=args, bits=bits, table=table, bf_pos=obf.set_positions(), ctx_pos=octx.set_positions(), bf_counts=obf.counts().copy(),
                keys=sorted(k_ for k_, _ in omap.items()), map=dict(omap.items()), cov=cov, g1=g1, g2=g2, gq=gq, kmers=stats["kmers"],
                general=want_general, tier3=want_tier3)
    return panel, want


def indexed(ctx, panel, want, scan=True):
    """index, reference scan and k-mer scan on the device, each against the oracle's; -> the resident panel"""
    ctx.reference_upload(panel.genome)
    rp = ResidentPanel(panel, 0, haploid=False)
    assert rp.index(ctx).sum() == 0
    ctx.bf_finalize(BF_ALT)
    for b, l in zip(panel.contig_base, panel.contig_len):
        ctx.ref_scan_resident(int(b), int(l))
    ctx.bf_finalize(BF_CTX)
    assert np.array_equal(ctx.bf_export_sparse(BF_ALT)[2], want["bf_pos"])
    assert np.array_equal(ctx.bf_export_sparse(BF_CTX)[2], want["ctx_pos"])
    assert sorted(ctx.map_export()[0]) == want["keys"]
    if scan:
        ctx.kmc_scan(*want["table"])
        assert np.array_equal(ctx.bf_export(BF_ALT)[3], want["bf_counts"])
        assert map_values_by_key(ctx) == want["map"]
    return rp


def check_settings(name):
    panel, want = setup(name)
    seen = []
    with Context(K, REF_K, want["bits"]) as ctx:
        ctx.set_option("use_record_counters", 2)              # (the lookups read the records' own copies, as at whole-genome size)
        rp = indexed(ctx, panel, want)
        for tiles in SETTINGS:
            ctx.set_option("lone_tiles", tiles)
            assert ctx.get_option("lone_tiles") == tiles
            rp.cov.zero_()
            rp.overflow.fill_(1)                              # (the call clears the flags itself)
            rp.call_step(ctx)
            got = rp.results()
            counts = ctx.blocks_stats()[3:7]
            print("%s lone_tiles=%d: general %d, lone k-mers %d, general k-mers %d, tier 3 %d; oracle k-mers %d"
                  % (name, tiles, counts[0], counts[1], counts[2], counts[3], want["kmers"]))
            assert np.array_equal(got["blk_var_off"], want["args"]["blk_var_off"])
            assert not got["overflow"].any()
            assert np.array_equal(got["cov"], want["cov"]), "lone_tiles=%d: first differing slot %d" % (tiles, np.flatnonzero(got["cov"] != want["cov"])[0])
            assert np.array_equal(got["g1"], want["g1"]) and np.array_equal(got["g2"], want["g2"]) and np.array_equal(got["gq"], want["gq"])
            assert counts[0] == want["general"] and counts[3] == want["tier3"]
            assert counts[1] + counts[2] == want["kmers"]     # signature k-mers looked up: tier 1's and the other tiers' together
            seen.append((counts, {key: got[key].copy() for key in ("cov", "overflow", "g1", "g2", "gq", "status")}))
    for counts, arrays in seen[1:]:
        assert counts == seen[0][0]
        for key, x in arrays.items():
            assert np.array_equal(x, seen[0][1][key]), key


@pytest.mark.parametrize("n", SEAMS)
def test_lone_snp_panels_at_the_tile_seams(n):
    check_settings(str(n))


def test_mixed_panel_lists_from_several_tiles():
    check_settings("mixed")


def test_overflow_flags_at_an_odd_address():
    """the cover call zeroes the caller's n flag bytes in one kernel with sixteen-byte stores between unaligned ends: flags that
    start three bytes into an allocation (1,125 records: a head of 13 bytes, 69 stores, a tail of 8) are all cleared, and the
    bytes before and behind them stay as they were"""
    panel, want = setup("mixed")
    with Context(K, REF_K, want["bits"]) as ctx:
        rp = indexed(ctx, panel, want)
        n, off = panel.n, 3
        flags = torch.full((n + 32,), 7, dtype=torch.uint8, device=rp.dev_t)
        rp.cut(ctx)
        ctx.cover_blocks_device(rp.dev, rp.blk_var_off.data_ptr(), rp.var_block.data_ptr(), rp.n_blocks.data_ptr(), False, rp.cov.data_ptr(), flags.data_ptr() + off)
        torch.cuda.synchronize()
        got = flags.cpu().numpy()
        assert flags.data_ptr() % 16 == 0 and (got[:off] == 7).all() and (got[off + n:] == 7).all() and not got[off:off + n].any()
        assert np.array_equal(rp.cov[:rp.n_slots].cpu().numpy().view(np.uint32), want["cov"])


def test_cohort_planes_equal_the_single_sample_call():
    """two planes (the table, and the table with other counts) through cohort_lone_kernel with one tile and with eight"""
    panel, want = setup("mixed")
    hi, lo, cnt = want["table"]
    tables = [(hi, lo, cnt), (hi[::2], lo[::2], (cnt[::2] % 7 + 1).astype(np.uint32))]
    dev = torch.device("cuda", 0)
    d_tables = [tuple(torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).to(dev) for a in map(np.ascontiguousarray, t)) for t in tables]

    def scan(ctx, s):
        h, l, c = d_tables[s]
        ctx.kmc_scan_device(h.data_ptr(), l.data_ptr(), c.data_ptr(), h.numel())

    keys = ("cov", "overflow", "g1", "g2", "gq", "status")
    with Context(K, REF_K, want["bits"]) as ctx:
        ctx.set_option("use_record_counters", 2)
        rp = indexed(ctx, panel, want, scan=False)
        single = []
        for s in range(2):
            ctx.counters_reset()
            scan(ctx, s)
            rp.call_step(ctx)
            r = rp.results()
            single.append({key: r[key].copy() for key in keys})
        assert np.array_equal(single[0]["cov"], want["cov"]) and not np.array_equal(single[0]["cov"], single[1]["cov"])
        co = ResidentCohort(rp, ctx, 2)
        for s in range(2):
            co.select(s)
            scan(ctx, s)
        for tiles in (1, 8):
            ctx.set_option("lone_tiles", tiles)
            co.cov.zero_()
            rp.overflow.fill_(1)
            co.call_step()
            for s in range(2):
                got = co.results(s)
                for key in keys:
                    assert np.array_equal(got[key], single[s][key]), "lone_tiles=%d, plane %d: %s differs" % (tiles, s, key)
        co.close()


@pytest.mark.parametrize("tiles", [1, 8])
def test_index_leaves_the_same_bits_and_map(tiles):
    """mg_index_blocks_device (panel_lone_index_kernel, a thread per record: a tile is 256 records) on the mixed panel and on the
    SNP panel one record beyond eight of ITS tiles"""
    for name in ("mixed", "1025"):
        panel, want = setup(name)
        with Context(K, REF_K, want["bits"]) as ctx:
            ctx.set_option("lone_tiles", tiles)
            indexed(ctx, panel, want, scan=False)
    big = synth.flat_from_snp_panel(synth.snp_panel(8 * 256 + 1, seed=77))
    args = oracle_blocks(big, K)
    obf, omap = ocapi.BF(1 << 22), ocapi.KMAP()
    ocapi.index_blocks(obf, omap, big.genome, **args, haploid=False, k=K)
    obf.switch_mode()
    with Context(K, REF_K, 1 << 22) as ctx:
        ctx.set_option("lone_tiles", tiles)
        ctx.reference_upload(big.genome)
        rp = ResidentPanel(big, 0, haploid=False)
        assert rp.index(ctx).sum() == 0
        ctx.bf_finalize(BF_ALT)
        assert np.array_equal(ctx.bf_export_sparse(BF_ALT)[2], obf.set_positions())
        keys, vals = ctx.map_export()
        assert sorted(keys) == sorted(k_ for k_, _ in omap.items()) and len(keys) == len(set(keys)) and not vals.any()


def test_lone_tiles_takes_0_1_2_4_8_only():
    with Context(K, REF_K, 1 << 16) as ctx:
        assert ctx.get_option("lone_tiles") == 0
        for bad in (-1, 3, 5, 16):
            with pytest.raises(MalvaError):
                ctx.set_option("lone_tiles", bad)
        assert ctx.get_option("lone_tiles") == 0


def test_slow_redo_strides_over_more_groups_than_its_grid():
    """140,000 lone SNPs, one tile per workgroup: 1,094 groups, more than the redo kernel's grid of four workgroups a CU, so its
    workgroups stride on.  Bases outside ACGT inside the windows of 300 of the first and 300 of the last 5,000 records mark their
    alleles for the redo; a mark the redo did not reach would stand in the coverages.  Index from the oracle with made-up weights
    (tests/test_gpu_resident.py's way); with eight tiles (137 groups, no stride) the same coverages."""
    bits = 1 << 26
    panel = synth.flat_from_snp_panel(synth.snp_panel(140_000, seed=91))
    rng = np.random.default_rng(9)
    gpos = panel.gpos()
    for v in np.concatenate([rng.choice(5_000, size=300, replace=False), panel.n - 1 - rng.choice(5_000, size=300, replace=False)]):
        panel.genome[int(gpos[v]) + int(rng.integers(-15, 16))] = ord("N")
    args = oracle_blocks(panel, K)
    obf, omap = ocapi.BF(bits), ocapi.KMAP()
    ocapi.index_blocks(obf, omap, panel.genome, **args, haploid=False, k=K)
    obf.switch_mode()
    cnts = obf.counts()
    cnts[:] = (1 + (np.arange(cnts.size, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(97)).astype(np.uint16)
    acgt = set(b"ACGT")
    for key, _ in list(omap.items()):
        if set(key) <= acgt:
            omap.increment(key, 1 + ocapi.xxh3_64(key) % 97)
    want_cov = ocapi.cover_blocks(obf, omap, panel.genome, **args, haploid=False, k=K)
    items = [(k_, v_) for k_, v_ in omap.items() if set(k_) <= acgt]
    seen = []
    with Context(K, REF_K, bits) as ctx:
        ctx.bf_import_sparse(BF_ALT, 1, bits, obf.set_positions(), obf.counts())
        ctx.bf_import_sparse(BF_CTX, 1, bits, np.zeros(0, np.uint64), np.zeros(0, np.uint16))
        ctx.map_import([k_ for k_, _ in items], np.array([v for _, v in items], dtype=np.int32))
        ctx.reference_upload(panel.genome)
        rp = ResidentPanel(panel, 0, haploid=False)
        for tiles in (1, 8):
            ctx.set_option("lone_tiles", tiles)
            rp.cov.zero_()
            rp.call_step(ctx)
            got = rp.results()
            assert not got["overflow"].any() and ctx.blocks_stats()[3] == 0       # every record is tier 1's
            assert np.array_equal(got["cov"], want_cov), "lone_tiles=%d: first differing slot %d" % (tiles, np.flatnonzero(got["cov"] != want_cov)[0])
            seen.append(got["cov"].copy())
    assert (want_cov > 0).sum() > 250_000 and (want_cov == 0).sum() >= 500      # (the planted bases do sit in windows: those alleles count nothing)
    assert np.array_equal(seen[0], seen[1])
