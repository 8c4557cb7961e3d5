"""The three tables made from the site words of `call --cohort` -- --ld (mg_pack_site_dosage, mg_ld_window), --ibd (mg_sites_to_planes,
mg_ibd_step) and --grm (mg_grm_step) -- on the seam cases of tests/ld_cases.py, ibd_cases.py and grm_cases.py: a pair, a break, a cell or a
run on every seam of slab, tile, chunk of groups, trip of the chunk loop, start word, tile of pairs and run plan.  The _cpu tests of the
three tables prove that each case holds what it claims, that its decoys alone change nothing and that its expectation is the
restatements'.  Every case goes through the host form and the device form, the device form into poisoned buffers between guard words
wherever the call has an output buffer (the GRM keeps its sums in the library's own state and hands them out through mg_grm_read).  Every
comparison is exact: integers, and r2 bit for bit."""
import numpy as np
import pytest
import torch

import grm_cases
import grm_model
import ibd_cases
import ld_cases
from ibd_model import IBD_SEG, IbdModel, ibd_segments, sort_segments
from ld_model import ld_pairs, site_words
from malva_amd import Context, MalvaError
from test_gpu_ibd import _same as _same_segs
from test_gpu_ld import _dev, _device_window, _same as _same_pairs

pytestmark = pytest.mark.gpu
MG_ERR_LIMIT = -5
POISON = 0xDEADBEEFDEADBEEF
PAD = 8


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def _guarded(words, fill=POISON):
    """a device buffer of `words` 64-bit words of poison between PAD guard words -> (tensor, pointer to the first word)"""
    t = _dev(np.full(words + 2 * PAD, fill, dtype=np.uint64))
    return t, t.data_ptr() + 8 * PAD


def _inside(t, words, what):
    h = t.cpu().numpy().view(np.uint64)
    assert (h[:PAD] == POISON).all() and (h[PAD + words:] == POISON).all(), "written outside %s" % what
    return h[PAD:PAD + words].copy()


# ---- LD: the window -------------------------------------------------------------------------------------------------------------------

LD_SEAMS = ld_cases.seam_cases()


@pytest.mark.parametrize("case", LD_SEAMS, ids=[c["name"] for c in LD_SEAMS])
def test_ld_window_on_a_seam_case(ctx, case):
    p = case["params"]
    args = (p["n_first"], p["window"], p["max_bp"], p["min_n"], p["min_r2"])
    want, want_off = ld_pairs(case["words"], case["chrom"], case["pos"], **p)
    k = len(want)
    assert [(int(x["i"]), int(x["j"])) for x in want] == case["pairs"]
    got, off = ctx.ld_window(case["words"], case["chrom"], case["pos"], p["window"], n_first=p["n_first"], max_bp=p["max_bp"], min_n=p["min_n"], min_r2=p["min_r2"])
    assert [(int(x["i"]), int(x["j"])) for x in got] == case["pairs"], "host form: the emitted pairs are not the claimed ones"
    _same_pairs(got, want)
    assert np.array_equal(off, want_off)
    rc, need, pairs, off = _device_window(ctx, case["words"], case["chrom"], case["pos"], *args, k)                    # the buffer exact, between guard words
    assert (rc, need) == (0, k) and np.array_equal(off, want_off)
    assert [(int(x["i"]), int(x["j"])) for x in pairs] == case["pairs"], "device form: the emitted pairs are not the claimed ones"
    _same_pairs(pairs, want)
    for cap in case["caps"] + [k - 1]:                                                                                 # pairs_cap inside a slab's ballot; one less
        rc, need, pairs, off = _device_window(ctx, case["words"], case["chrom"], case["pos"], *args, cap)
        assert (rc, need) == (MG_ERR_LIMIT, k) and np.array_equal(off, want_off)
        _same_pairs(pairs, want[:cap])
        with pytest.raises(MalvaError) as e:
            ctx.ld_window(case["words"], case["chrom"], case["pos"], p["window"], n_first=p["n_first"], max_bp=p["max_bp"], min_n=p["min_n"], min_r2=p["min_r2"], pairs_cap=cap)
        assert e.value.code == MG_ERR_LIMIT and e.value.needed == k
        _same_pairs(e.value.pairs[:cap], want[:cap])
        assert not e.value.pairs[cap:].view(np.uint8).any(), "written at or behind pairs_cap"


@pytest.mark.parametrize("plane,record,dosage", ld_cases.pack_cases())
def test_pack_site_dosage_on_one_cell_among_decoys(ctx, plane, record, dosage):
    g1, g2, gq, vao = ld_cases.pack_case(plane, record, dosage)
    n, q = ld_cases.PACK_N, ld_cases.PACK_MIN_GQ
    want = site_words(g1, g2, gq, False, vao, q)
    assert [int(x != 0) for x in want.reshape(-1)].count(1) == 1 and int(want[dosage, record]) == 1 << plane, "exactly one bit"
    got = ctx.pack_site_dosage(g1, g2, gq, False, vao, min_gq=q, out=np.full((3, n), POISON, dtype=np.uint64))
    assert np.array_equal(got, want), "host form"
    d1, d2, dq, dv = _dev(g1), _dev(g2), _dev(gq), _dev(vao)
    out, ptr = _guarded(3 * n)
    torch.cuda.synchronize()
    ctx.pack_site_dosage_device(n, 64, False, d1.data_ptr(), d2.data_ptr(), dq.data_ptr(), dv.data_ptr(), ptr, min_gq=q)
    ctx.synchronize()
    assert np.array_equal(_inside(out, 3 * n, "the words").reshape(3, n), want), "device form"


# ---- IBD: the transpose, the starts, the walk ---------------------------------------------------------------------------------------------

IBD_SEAMS = ibd_cases.seam_cases()


def _model_steps(case, cuts):
    """the model cut as the walk is cut -> the segments of every step"""
    m = IbdModel(case["n_samples"], case["min_records"], case["min_bp"])
    edges = [0] + list(cuts) + [case["D"].shape[0]]
    return [m.step(case["D"][c0:c1], case["chrom"][c0:c1], case["pos"][c0:c1], flush=i == len(edges) - 2) for i, (c0, c1) in enumerate(zip(edges[:-1], edges[1:]))]


def _walk_exact(ctx, case, cuts, device):
    """begin, one step per piece of `cuts` with segs_cap exactly what the step closes, a last step of no records that flushes again (nothing
    is open: it closes nothing), end -> the steps' outputs.  device: through mg_ibd_step_device into a poisoned buffer between guard words;
    else through the host form into a poisoned array, which stays poison behind the step's segments"""
    steps = _model_steps(case, cuts)
    n, G = case["D"].shape[0], case["words"].shape[0]
    edges = [0] + list(cuts) + [n]
    ctx.ibd_begin(case["n_samples"], case["min_records"], case["min_bp"])
    parts = []
    for i, (c0, c1) in enumerate(zip(edges[:-1], edges[1:])):
        need, flush = len(steps[i]), i == len(edges) - 2
        w, ch, po = np.ascontiguousarray(case["words"][:, :, c0:c1]), case["chrom"][c0:c1], case["pos"][c0:c1]
        if device:
            ds, dc, dp = _dev(w), _dev(ch), _dev(po)
            out, ptr = _guarded(4 * need)
            torch.cuda.synchronize()
            rc, got_need = ctx.ibd_step_device(c1 - c0, G, ds.data_ptr(), dc.data_ptr(), dp.data_ptr(), flush, ptr, need)
            ctx.synchronize()
            assert (rc, got_need) == (0, need), "step %d of %s" % (i, cuts)
            seg = _inside(out, 4 * need, "the segments' buffer").view(IBD_SEG)
        else:
            buf = np.full(4 * (need + PAD), POISON, dtype=np.uint64).view(IBD_SEG)
            seg = ctx.ibd_step(w, ch, po, flush=flush, segs_cap=need, segs=buf)
            assert len(seg) == need and (buf.view(np.uint64)[4 * need:] == POISON).all(), "written behind segs_cap"
        _same_segs(seg.copy(), steps[i])                                           # (step by step: ordered by (a, b), every pair's at its own offset)
        parts.append(seg.copy())
    again = ctx.ibd_step(case["words"][:, :, :0], case["chrom"][:0], case["pos"][:0], flush=True, segs_cap=0)
    assert len(again) == 0, "a flush with nothing open closes nothing"
    ctx.ibd_end()
    return sort_segments(parts)


@pytest.mark.parametrize("case", IBD_SEAMS, ids=[c["name"] for c in IBD_SEAMS])
def test_ibd_steps_on_a_seam_case(ctx, case):
    want = ibd_segments(case["D"], case["chrom"], case["pos"], case["n_samples"], case["min_records"], case["min_bp"])
    if case["expect"] is not None:
        assert [tuple(int(s[f]) for f in ("chrom", "start_pos", "end_pos", "n", "ibs2")) for s in want] == case["expect"]
    for cuts in case["cuts"]:
        _same_segs(_walk_exact(ctx, case, cuts, device=False), want)
    for cuts in case["cuts"][:2]:                                                  # (the uncut walk and the first cut, which is the one at the seam)
        _same_segs(_walk_exact(ctx, case, cuts, device=True), want)


@pytest.mark.parametrize("sample", ibd_cases.TR_SAMPLES)
def test_transpose_of_one_cell_and_its_decoy(ctx, sample):
    for record in ibd_cases.TR_RECORDS:
        words, want = ibd_cases.transpose_case(sample, record)
        got = ctx.sites_to_planes(words, out=np.full(want.shape, POISON, dtype=np.uint64))
        assert np.array_equal(got, want), "host form, record %d" % record
        ds = _dev(words)
        out, ptr = _guarded(want.size)
        torch.cuda.synchronize()
        ctx.sites_to_planes_device(ibd_cases.TR_N, 3, ds.data_ptr(), ptr)
        ctx.synchronize()
        assert np.array_equal(_inside(out, want.size, "the planes").reshape(want.shape), want), "device form, record %d" % record


# ---- GRM: the Gram kernel without atomics, a full run of the i32 accumulators ------------------------------------------------------------

GRM_PLANS = grm_cases.plan_cases()


def _grm_equal(got, want, what):
    assert got[2:] == want[2:], "%s: records seen, entered: %s, expected %s" % (what, got[2:], want[2:])
    for k, name in ((1, "N"), (0, "S")):
        if not np.array_equal(got[k], want[k]):
            at = int(np.flatnonzero(got[k] != want[k])[0])
            a, b = (int(x[at]) for x in grm_model.pair_index(int(round((np.sqrt(8 * len(want[k]) + 1) - 1) / 2))))
            raise AssertionError("%s: %s differs in %d pairs, first at (%d, %d): %d, expected %d" % (what, name, int((got[k] != want[k]).sum()), a, b, int(got[k][at]),
                                                                                                    int(want[k][at])))


@pytest.mark.parametrize("case", GRM_PLANS, ids=[c["name"] for c in GRM_PLANS])
def test_grm_step_on_a_plan_case(ctx, case):
    """one step under the default cap of 384 MiB, so that the library cuts it as the case's plan says (tests/test_grm_cases_cpu.py)"""
    assert ctx.get_option("grm_scratch_mb") == 384
    n = case["n_samples"]
    words = grm_cases.plan_case_words(case)
    want = grm_cases.plan_case_expected(case)
    ctx.grm_begin(n, case["haploid"], case["maf_ppm"], case["min_n"])
    ctx.grm_step(words)
    _grm_equal(ctx.grm_read(n), want, "host form")
    ds = _dev(words)
    torch.cuda.synchronize()
    ctx.grm_begin(n, case["haploid"], case["maf_ppm"], case["min_n"])
    ctx.grm_step_device(words.shape[2], words.shape[0], ds.data_ptr())
    _grm_equal(ctx.grm_read(n), want, "device form")
    ctx.grm_end()
