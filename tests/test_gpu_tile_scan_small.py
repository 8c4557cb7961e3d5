"""launch_tile_scan with one workgroup's worth of tile sums (up to SCAN_CHUNK = 8,192: tile_scan_small_kernel, one launch) and one
more (the reduce / part scan / rescan triple), through its two nearest callers: the block cut of the record loop
(mg_cut_blocks_device: a tile is 256 records) and the filters' rank directory (mg_bf_finalize behind a sparse import: a tile is
256 blocks of 512 bits).  The scan by itself at these sizes is tests/test_gpu_store_edges.py's.  Everything is exact."""
import numpy as np
import pytest
import torch

import store_cases as sc
from malva_amd import BF_CTX, Context
from malva_amd.capi import PanelDev, rows_of
from oracle import capi as ocapi

pytestmark = pytest.mark.gpu

K = 35
TPB, SCAN_CHUNK = 256, 8192           # a test's copy of csrc/store_kernels.h
N_TILES = [1, 2, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1]


@pytest.fixture(scope="module")
def ctx():
    c = Context(K, 43, 1 << 16)
    yield c
    c.close()


def _positions(n, seed):
    """SNPs on two sequences, gaps of 1..60 nt: about half of the records start a block at k = 35, so a tile's count is anything
    from a few to 256 and the prefix differs from tile to tile"""
    rng = np.random.default_rng(seed)
    cid = np.zeros(n, dtype=np.uint32)
    cid[n - n // 3:] = 1
    pos = np.cumsum(rng.integers(1, 61, size=n)).astype(np.int64)
    pos[cid == 1] -= pos[n - n // 3] - 5                      # the second sequence starts over at 5
    return pos.astype(np.int32), cid


@pytest.mark.parametrize("n_tiles", N_TILES)
def test_cut_blocks_device_at_the_single_workgroup_seam(ctx, n_tiles):
    n = TPB * n_tiles
    pos, cid = _positions(n, seed=n_tiles)
    ones = np.ones(n, dtype=np.uint32)
    off, _ = ocapi.cut_blocks(pos, ones, ones, cid, K)
    heads = np.zeros(n, dtype=np.int64)
    heads[off[:-1].astype(np.int64)] = 1
    want_block = np.cumsum(heads) - 1                         # the scan, restated: the block of record v is the heads up to v, less one
    want_off = np.append(np.flatnonzero(heads), n)
    assert len(want_off) - 1 > n // 4 and heads.sum() < n     # blocks of one and of several
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)
    t = {"pos": up(pos), "ref_size": up(ones), "min_size": up(ones), "contig_id": up(cid)}
    d = PanelDev()
    d.n_vars = n
    for name, x in t.items():
        setattr(d, name, x.data_ptr())
    blk_var_off = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    var_block = torch.full((n,), -1, dtype=torch.int32, device=dev)
    n_blocks = torch.full((1,), -1, dtype=torch.int64, device=dev)
    for again in range(2):                                    # the tile sums are scanned in place: a second call starts from fresh ones
        ctx.cut_blocks_device(d, blk_var_off.data_ptr(), var_block.data_ptr(), n_blocks.data_ptr())
        torch.cuda.synchronize()
        nb = int(n_blocks.item())
        assert nb == len(want_off) - 1
        assert np.array_equal(blk_var_off[:nb + 1].cpu().numpy().astype(np.int64), want_off)
        assert np.array_equal(var_block.cpu().numpy().astype(np.int64), want_block)


@pytest.mark.parametrize("size", [sc.CHUNK_BITS - 512, sc.CHUNK_BITS], ids=["8192-tiles", "8193-tiles"])
def test_rank_directory_on_either_side_of_the_seam(size):
    """2^30 - 512 bits are 8,192 tiles of the directory's scan (with the total's entry), 2^30 bits 8,193: set bits at both ends of
    the blocks around every seam the table names, 20,000 elsewhere, a counter of its own per rank"""
    assert sc.geometry(size)[2] == (SCAN_CHUNK if size < sc.CHUNK_BITS else SCAN_CHUNK + 1)
    c = sc.filter_case("%d-edges" % size)
    obf = sc.oracle_filter(c.size, c.pos, c.counts)
    with Context(sc.K, 43, size) as ctx:
        ctx.bf_import_sparse(BF_CTX, 1, c.size, c.pos, c.counts)
        assert ctx.bf_info(BF_CTX) == (c.size, len(c.pos), 1)
        _, _, pos, counts = ctx.bf_export_sparse(BF_CTX)
        assert np.array_equal(pos, c.pos) and np.array_equal(counts, obf.counts())
        got = ctx.bf_get_count(BF_CTX, rows_of(c.probe))
        want = np.array([obf.get_count(km) for km in c.probe], dtype=np.uint16)
        assert c.hits > 100 and np.array_equal(got, want)
