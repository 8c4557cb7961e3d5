"""mg_cells and mg_bcf_keys as the binding lays them out (capi.Cells, capi.BcfKeys) against the library's: one call that sets every member
at once -- the mask, COVS, GP and PL -- through all four row encoders, with arrays that differ in content wherever two members have the
same type, so that a member at the wrong offset or two swapped pointers give other bytes.

The expected rows are the existing restatements': tests/test_gpu_pl.py's (its generator, its text and BCF rows with tests/pl_model.py's
missing value, tests/bcf_writer.py's layout behind them) over tests/test_gpu_gp.py's text model."""
import ctypes as C

import numpy as np
import pytest

from malva_amd import Context
from malva_amd.capi import BcfKeys, Cells
from test_gpu_pl import _case, _device_rows, _rows_bcf, _rows_text

pytestmark = pytest.mark.gpu
MG_ERR_ARG = -1
FMT_ROWS = 32                                                                      # records per workgroup of the write pass
KEYS = (1, 130, 3, 40000, 5)                                                       # (every key its own value; int8, int16 and int32 among them)
MIN_GQ = 50


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def _distinct(planes, alleles, haploid):
    """test_gpu_pl's case with the arrays of one type made different in every element: gt2 != gt1 in every cell, gq on both sides of
    the mask and never an allele index, no coverage that is a PL value"""
    g1, g2, gq, cov, vao, probs, vgo, status, pl = _case(planes, alleles, haploid, seed=5 + planes + len(alleles))
    n = len(alleles)
    cell = np.arange(planes * n, dtype=np.int32).reshape(planes, n)
    g1[...] = cell % 3
    g2[...] = (cell + 1) % 3
    gq[...] = 10 + (cell * 37) % 90
    cov[...] = 100000 + np.arange(cov.size, dtype=np.uint32).reshape(cov.shape)
    return g1, g2, gq, cov, vao, probs, vgo, status, pl


@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("alleles", [[1], [3], [2, 1, 3] * ((FMT_ROWS + 1) // 3)], ids=["one-slot", "three-slots", "two-workgroups"])
def test_every_member_at_once(ctx, alleles, planes, haploid):
    assert len(alleles) in (1, FMT_ROWS + 1)
    case = g1, g2, gq, cov, vao, probs, vgo, status, pl = _distinct(planes, alleles, haploid)
    kw = dict(probs=probs, status=status, cov=cov, min_gq=MIN_GQ)
    host = {False: ctx.format_calls_pl(g1, g2, gq, haploid, vao, vgo, pl, **kw), True: ctx.encode_calls_bcf_pl(g1, g2, gq, haploid, KEYS, vao, vgo, pl, **kw)}
    for bcf in (False, True):
        want, want_off = _rows_bcf(case, haploid, KEYS, True, True, MIN_GQ) if bcf else _rows_text(case, haploid, True, True, MIN_GQ)
        got, off = host[bcf]
        assert np.array_equal(off, want_off) and got == want
        rc, need, out, guard, doff = _device_rows(ctx, bcf, case, haploid, KEYS, True, True, MIN_GQ, len(want), shift=3)
        assert rc == 0 and need == len(want) and (guard == 0xAA).all()
        assert out == got and np.array_equal(doff, off), "the host form and the device form disagree"
    if len(alleles) > 1:                                                           # what the case held: both sides of the mask, all four fields
        text = host[False][0]
        assert ((b"\t.:" in text) if haploid else (b"\t./.:" in text)) and (b"\t%d" % g1[0, 0]) in text and b":100000" in text


@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 3])
def test_no_record(ctx, planes, haploid):
    case = g1, g2, gq, cov, vao, probs, vgo, status, pl = _distinct(planes, [], haploid)
    kw = dict(probs=probs, status=status, cov=cov, min_gq=MIN_GQ)
    for got, off in (ctx.format_calls_pl(g1, g2, gq, haploid, vao, vgo, pl, **kw), ctx.encode_calls_bcf_pl(g1, g2, gq, haploid, KEYS, vao, vgo, pl, **kw)):
        assert got == b"" and list(off) == [0]
    for bcf in (False, True):
        rc, need, out, guard, doff = _device_rows(ctx, bcf, case, haploid, KEYS, True, True, MIN_GQ, 0)
        assert rc == 0 and need == 0 and list(doff) == [0] and (guard == 0xAA).all()


def test_a_null_struct_is_an_argument_error(ctx):
    need, off, buf = C.c_uint64(0), (C.c_uint64 * 1)(), (C.c_uint8 * 8)()
    x, k = Cells(0, 1, 0), BcfKeys(1, 2, 3, 4, 5)
    for entry in (ctx._L.mg_format_calls, ctx._L.mg_format_calls_device):
        assert entry(ctx.h, None, buf, 8, off, C.byref(need)) == MG_ERR_ARG
    for entry in (ctx._L.mg_encode_calls_bcf, ctx._L.mg_encode_calls_bcf_device):
        assert entry(ctx.h, None, C.byref(k), buf, 8, off, C.byref(need)) == MG_ERR_ARG
        assert entry(ctx.h, C.byref(x), None, buf, 8, off, C.byref(need)) == MG_ERR_ARG
