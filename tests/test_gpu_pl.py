"""`call --cohort --merged --pl`: prior-free Phred-scaled genotype likelihoods, made on the device by mg_phred_likelihoods and written as
the FORMAT field PL by mg_format_calls (text) and mg_encode_calls_bcf (BCF2) under MG_CELLS_PL.

The values are held against tests/pl_model.py, which tests/test_pl_cpu.py pins to the oracle; the rows against a restatement built here on
what the tests of the entries without PL pin (test_gpu_merged.format_plain, test_gpu_bcf.encode_plain, test_gpu_gp.expect_text /
expect_bcf).  Every comparison is exact."""
import ctypes as C
import functools
import os
import struct

import numpy as np
import pytest
import torch

import pl_model
from malva_amd import Context, MalvaError
from malva_amd.capi import CELLS_GP, CELLS_PL, BcfKeys, Cells
from test_bcf_out_cpu import bcf_to_vcf, bgzf_members
from test_gpu_bcf import PACK, desc, encode_plain, int_type, typed_int
from test_gpu_gp import _records, _run, cohorts, expect_bcf, expect_text, n_gt  # noqa: F401 (cohorts: the fixture of the two small cohorts)
from test_gpu_merged import format_plain

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE, MG_ERR_LIMIT = -1, -3, -5
M = pl_model.MISSING
INT32_MAX = 2 ** 31 - 1
MAX_COV = 200
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


# ---- the values -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cells(n, planes, seed):
    """n records, A from 0, 1, 2, 3, 4, 8, 16 -- records 64 .. 127 (the second wave of a plane) all biallelic, the others mixed --, and
    their coverages: random, with planted cells that are all zero, exactly max_cov, max_cov + 1, and one allele dominant"""
    rng = np.random.default_rng(seed)
    pattern = [2, 2, 3, 2, 0, 2, 4, 2, 1, 2, 2, 8, 2, 3, 2, 2]
    A = np.array([2 if 64 <= v < 128 else pattern[v % 16] for v in range(n)], dtype=np.int64)
    if n > 40:
        A[[7, 39]] = 16
    if n == 1:
        A[0] = 3
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)
    low = rng.integers(0, 25, size=(planes, int(vao[-1])))
    cov = np.where(rng.random(size=low.shape) < 0.6, low, rng.integers(0, MAX_COV + 1, size=low.shape)).astype(np.uint32)
    for v in range(n):
        a0, a1 = int(vao[v]), int(vao[v + 1])
        if a1 == a0:
            continue
        for p in range(planes):
            kind = (v * 7 + p * 3) % 23
            if kind == 0:
                cov[p, a0:a1] = 0                                                   # no data
            elif kind == 1:
                cov[p, a0 + (v + p) % (a1 - a0)] = MAX_COV                          # exactly the most: genotyped
            elif kind == 2:
                cov[p, a0 + (v + p) % (a1 - a0)] = MAX_COV + 1                      # over-covered: missing
            elif kind == 3:
                cov[p, a0:a1] = 0
                cov[p, a0 + (v + p) % (a1 - a0)] = 150                              # one allele dominant
            elif kind == 4:
                cov[p, a0:a1] = rng.integers(0, 3, size=a1 - a0)                    # a read or two
    return A, vao, cov


@functools.lru_cache(maxsize=None)
def _want(n, planes, seed, haploid, error_rate, cap):
    A, vao, cov = _cells(n, planes, seed)
    return pl_model.pl_array(cov, vao, error_rate, MAX_COV, haploid, cap)


def _host(ctx, cov, vao, vgo, e, haploid, cap):
    P, ng = cov.shape[0], int(vgo[-1])
    buf = np.full(P * ng + 64, GUARD, dtype=np.int32)
    got, _ = ctx.phred_likelihoods(cov, vao, e, MAX_COV, haploid, cap=cap, var_gt_off=vgo, pl_out=buf[:P * ng].reshape(P, ng))
    assert (buf[P * ng:] == GUARD).all(), "the guard behind pl_out was written"
    return got


def _device(ctx, cov, vao, vgo, e, haploid, cap):
    dev = torch.device("cuda", 0)
    P, ng, n = cov.shape[0], int(vgo[-1]), len(vao) - 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)).reshape(-1).view(np.uint8)).to(dev)
    dc, dv, dg = t(cov), t(vao), t(vgo)
    out = torch.full((P * ng + 64,), GUARD, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.phred_likelihoods_device(n, P, dc.data_ptr(), dv.data_ptr(), dg.data_ptr(), e, MAX_COV, haploid, cap, out.data_ptr())
    ctx.synchronize()
    h = out.cpu().numpy()
    assert (h[P * ng:] == GUARD).all(), "the guard behind pl_out was written"
    return h[:P * ng].reshape(P, ng)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes,n", [(1, 1), (3, 255), (64, 257), (3, 1025), (1, 257)])
def test_likelihoods_are_the_model(ctx, planes, n, haploid, form):
    """n_vars on both sides of a workgroup (256) and past a grid of several; 1, 3 and 64 planes; a wave of mixed A and an all-biallelic one"""
    A, vao, cov = _cells(n, planes, 100 + n)
    want, vgo = _want(n, planes, 100 + n, haploid, 0.001, 255)
    got = (_host if form == "host" else _device)(ctx, cov, vao, vgo, 0.001, haploid, 255)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5]
    ms = ctx.pl_stats()
    assert np.isfinite(ms) and ms >= 0
    if n >= 255:                                                                   # what the data held
        per_cell = [want[p, int(vgo[v]):int(vgo[v + 1])] for p in range(planes) for v in range(n) if A[v]]
        assert any((c == M).all() for c in per_cell), "no missing cell"
        assert (want == 255).any(), "no value at the cap"
        assert any((c == 0).all() and len(c) > 1 for c in per_cell), "no all-zero cell"
        assert any(len(c) > 3 and (c != M).all() for c in per_cell), "no multi-allelic cell"
        assert (A[:64] != 2).any() and (A[64:128] == 2).all()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("error_rate,cap", [(0.001, 1), (0.001, INT32_MAX), (0.0, 255), (0.0, INT32_MAX), (1.0, 255), (0.25, 40)])
def test_caps_and_error_rates(ctx, error_rate, cap, haploid, form):
    planes, n = 3, 257
    A, vao, cov = _cells(n, planes, 7)
    want, vgo = _want(n, planes, 7, haploid, error_rate, cap)
    got = (_host if form == "host" else _device)(ctx, cov, vao, vgo, error_rate, haploid, cap)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    per_cell = [want[p, int(vgo[v]):int(vgo[v + 1])] for p in range(planes) for v in range(n) if A[v] > 1]
    if error_rate == 0.0 and not haploid:                                          # 0 * -inf = NaN beside finite values; -inf: the cap
        assert any((c == M).any() and not (c == M).all() for c in per_cell), "no individually missing value"
        assert (want == cap).any()
    if error_rate == 1.0:
        assert all((c == M).all() for c in per_cell)
    if cap == 1:
        assert set(np.unique(want)) == {M, 0, 1}
    if cap == INT32_MAX and error_rate == 0.001:
        assert want.max() > 255 and want.max() < INT32_MAX


def test_no_record_and_bad_arguments(ctx):
    vao, vgo = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    got, _ = ctx.phred_likelihoods(np.zeros((2, 0), dtype=np.uint32), vao, 0.001, MAX_COV, False)
    assert got.shape == (2, 0) and ctx.pl_stats() >= 0
    ctx.phred_likelihoods_device(0, 2, 0, 0, 0, 0.001, MAX_COV, False, 255, 0)
    ctx.synchronize()
    assert ctx.pl_stats() >= 0
    with Context(35, 43, 1 << 20) as fresh:
        with pytest.raises(MalvaError) as e:
            fresh.pl_stats()
        assert e.value.code == MG_ERR_STATE
    cov = np.full((1, 2), 5, dtype=np.uint32)
    vao, vgo = np.array([0, 2], dtype=np.uint32), np.array([0, 3], dtype=np.uint64)
    for bad in (dict(cap=0), dict(cap=-5), dict(planes=0), dict(planes=65), dict(vgo=np.array([0, 2], dtype=np.uint64))):
        out = np.full(3, GUARD, dtype=np.int32)
        rc = ctx._L.mg_phred_likelihoods(ctx.h, 1, bad.get("planes", 1), cov.ctypes.data_as(C.c_void_p), vao.ctypes.data_as(C.c_void_p),
                                         bad.get("vgo", vgo).ctypes.data_as(C.c_void_p), C.c_float(0.001), MAX_COV, 0, bad.get("cap", 255), out.ctypes.data_as(C.c_void_p))
        assert rc == MG_ERR_ARG and (out == GUARD).all(), bad
    assert ctx._L.mg_phred_likelihoods(ctx.h, 1, 1, None, vao.ctypes.data_as(C.c_void_p), vgo.ctypes.data_as(C.c_void_p), C.c_float(0.001), MAX_COV, 0, 255, None) == MG_ERR_ARG


# ---- the rows -------------------------------------------------------------------------------------------------------------------

POOL = [0, 9, 10, 119, 120, 127, 128, 32759, 32760, 32767, 32768, INT32_MAX, -1, -9, -10, -120, -121, -32760, -32761, -INT32_MAX, M + 1, 255, 99, 100, 1000]
MISS_T = {1: -128, 2: -32768, 3: M}


def pl_text(vals):
    return "." if not len(vals) or all(x == M for x in vals) else ",".join("." if x == M else str(x) for x in vals)


def pl_field(key, G, cells):
    """cells: per plane the G values -> the field's bytes"""
    real = [x for c in cells for x in c if x != M]
    t = int_type(min(real), max(real)) if real else 1
    out = typed_int(key) + desc(G, t)
    for c in cells:
        if G and all(x == M for x in c):
            c = [MISS_T[t]] + [MISS_T[t] + 1] * (G - 1)
        out += b"".join(struct.pack(PACK[t], MISS_T[t] if x == M else x) for x in c)
    return out


def _rows_text(case, haploid, with_gp, with_cov, min_gq):
    g1, g2, gq, cov, vao, probs, vgo, status, pl = case
    cov = cov if with_cov else None
    P, n = g1.shape
    if with_gp:
        base, off = expect_text(g1, g2, gq, haploid, vao, probs, vgo, status, cov, min_gq)
    else:
        base, off = format_plain(g1, g2, gq, haploid, cov, vao if cov is not None else None)
    rows = [base[int(off[v]):int(off[v + 1])].decode()[1:-1].split("\t") for v in range(n)]
    if not with_gp and min_gq is not None:
        rows = [[("." if haploid else "./.") + c[c.index(":"):] if int(gq[p, v]) < min_gq else c for p, c in enumerate(r)] for v, r in enumerate(rows)]
    out = [("".join("\t" + c + ":" + pl_text([int(x) for x in pl[p, int(vgo[v]):int(vgo[v + 1])]]) for p, c in enumerate(rows[v])) + "\n").encode() for v in range(n)]
    o = np.zeros(n + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(r) for r in out])
    return b"".join(out), o


def _rows_bcf(case, haploid, keys, with_gp, with_cov, min_gq):
    g1, g2, gq, cov, vao, probs, vgo, status, pl = case
    cov = cov if with_cov else None
    P, n = g1.shape
    if with_gp:
        base, off = expect_bcf(g1, g2, gq, haploid, keys[:4], vao, probs, vgo, status, cov, min_gq)
    else:
        base, off = encode_plain(g1, g2, gq, haploid, keys[:3], cov, vao, min_gq)
    out = []
    for v in range(n):
        G = int(vgo[v + 1]) - int(vgo[v])
        out.append(base[int(off[v]):int(off[v + 1])] + pl_field(keys[4], G, [[int(x) for x in pl[p, int(vgo[v]):int(vgo[v + 1])]] for p in range(P)]))
    o = np.zeros(n + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(r) for r in out])
    return b"".join(out), o


def _case(planes, alleles, haploid, seed):
    rng = np.random.default_rng(seed)
    n = len(alleles)
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(alleles)
    vgo = np.zeros(n + 1, dtype=np.uint64)
    vgo[1:] = np.cumsum([n_gt(a, haploid) for a in alleles])
    g1, g2 = (rng.integers(0, 3, size=(planes, n)).astype(np.int32) for _ in range(2))
    gq = rng.integers(0, 100, size=(planes, n)).astype(np.int32)
    cov = rng.integers(0, 300, size=(planes, int(vao[-1]))).astype(np.uint32)
    probs = rng.random(size=(planes, int(vgo[-1])))
    status = np.where(rng.random(size=(planes, n)) < 0.2, rng.integers(1, 4, size=(planes, n)), 0).astype(np.uint8)
    status[:, np.asarray(alleles) == 0] = 0                                        # (a record without alleles has an empty list, which is a list)
    pl = rng.integers(0, 256, size=(planes, int(vgo[-1]))).astype(np.int64)
    edge = rng.random(size=pl.shape) < 0.15
    pl[edge] = np.array(POOL, dtype=np.int64)[rng.integers(0, len(POOL), size=int(edge.sum()))]
    pl[rng.random(size=pl.shape) < 0.1] = M                                        # single values missing
    for p in range(planes):                                                        # whole cells missing
        for v in range(n):
            if (p + 3 * v) % 11 == 0:
                pl[p, int(vgo[v]):int(vgo[v + 1])] = M
    return g1, g2, gq, cov, vao, probs, vgo, status, pl.astype(np.int32)


def _device_rows(ctx, bcf, case, haploid, keys, with_gp, with_cov, min_gq, cap, guard=64, shift=0):
    g1, g2, gq, cov, vao, probs, vgo, status, pl = case
    dev = torch.device("cuda", 0)
    P, n = g1.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)).reshape(-1).view(np.uint8)).to(dev)
    d1, d2, dq, dc, dv, dp, dg, ds, dl = (t(a) for a in (g1, g2, gq, cov if with_cov else None, vao, probs if with_gp else None, vgo, status if with_gp else None, pl))
    out = torch.full((shift + cap + guard,), 0xAA, dtype=torch.uint8, device=dev)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ptr = lambda x: 0 if x is None else x.data_ptr()
    dst = out.data_ptr() + shift if cap else 0
    if bcf:
        rc, need = ctx.encode_calls_bcf_pl_device(n, P, haploid, ptr(d1), ptr(d2), ptr(dq), ptr(dc), ptr(dv), ptr(dp), ptr(dg), ptr(ds), ptr(dl), keys, dst, cap,
                                                  off.data_ptr(), min_gq=min_gq)
    else:
        rc, need = ctx.format_calls_pl_device(n, P, haploid, ptr(d1), ptr(d2), ptr(dq), ptr(dc), ptr(dv), ptr(dp), ptr(dg), ptr(ds), ptr(dl), dst, cap, off.data_ptr(),
                                              min_gq=min_gq)
    ctx.synchronize()
    h = out.cpu().numpy()
    assert (h[:shift] == 0xAA).all(), "bytes in front of the buffer were written"
    return rc, need, h[shift:shift + cap].tobytes(), h[shift + cap:], off.cpu().numpy().view(np.uint64)


def _both(ctx, case, haploid, keys=(1, 2, 3, 4, 5), with_gp=False, with_cov=False, min_gq=None, shifts=(0, 7)):
    g1, g2, gq, cov, vao, probs, vgo, status, pl = case
    want_t, off_t = _rows_text(case, haploid, with_gp, with_cov, min_gq)
    want_b, off_b = _rows_bcf(case, haploid, keys, with_gp, with_cov, min_gq)
    kw = dict(probs=probs if with_gp else None, status=status if with_gp else None, cov=cov if with_cov else None, min_gq=min_gq)
    got, off = ctx.format_calls_pl(g1, g2, gq, haploid, vao, vgo, pl, **kw)
    assert np.array_equal(off, off_t) and got == want_t
    assert all(np.isfinite(m) and m >= 0 for m in ctx.format_stats())
    got, off = ctx.encode_calls_bcf_pl(g1, g2, gq, haploid, keys, vao, vgo, pl, **kw)
    assert np.array_equal(off, off_b) and got == want_b
    assert all(np.isfinite(m) and m >= 0 for m in ctx.bcf_stats())
    for shift in shifts:
        for bcf, want, want_off in ((False, want_t, off_t), (True, want_b, off_b)):
            rc, need, out, guard, doff = _device_rows(ctx, bcf, case, haploid, keys, with_gp, with_cov, min_gq, len(want), shift=shift)
            assert rc == 0 and need == len(want) and np.array_equal(doff, want_off)
            assert out == want and (guard == 0xAA).all()
    return want_t, want_b


def test_the_restatement_knows_the_edges():
    assert pl_text([]) == "." and pl_text([M, M]) == "." and pl_text([M, 0, -7]) == ".,0,-7" and pl_text([M + 1]) == str(M + 1)
    assert pl_field(5, 0, [[], []]) == b"\x11\x05\x01"
    assert pl_field(5, 3, [[M, M, M], [1, M, 127]]) == b"\x11\x05\x31" + bytes([0x80, 0x81, 0x81, 1, 0x80, 127])
    assert pl_field(5, 2, [[M, M], [M, M]]) == b"\x11\x05\x21" + bytes([0x80, 0x81, 0x80, 0x81])            # no value at all: int8
    assert pl_field(5, 1, [[128], [M]]) == b"\x11\x05\x12" + struct.pack("<hH", 128, 0x8000)
    assert pl_field(5, 2, [[M, M], [0, 32768]]) == b"\x11\x05\x23" + struct.pack("<IIii", 0x80000000, 0x80000001, 0, 32768)
    assert pl_field(5, 1, [[M + 1]])[2] == 0x13 and pl_field(5, 1, [[-120]])[2] == 0x11 and pl_field(5, 1, [[-121]])[2] == 0x12


@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
def test_one_value_decides_the_type(ctx, haploid):
    """a record per pool value: every value of the record is 5 but one, the last of the last plane; G = 3 (diploid) or 2"""
    planes, n = 3, len(POOL)
    case = list(_case(planes, [2] * n, haploid, seed=1))
    vgo, pl = case[6], case[8]
    pl[:] = 5
    for v, x in enumerate(POOL):
        pl[planes - 1, int(vgo[v + 1]) - 1] = x
    text, bcf = _both(ctx, case, haploid)
    G = 2 if haploid else 3
    for x, t in ((127, 1), (128, 2), (-120, 1), (-121, 2), (32767, 2), (32768, 3), (-32760, 2), (-32761, 3), (INT32_MAX, 3), (M + 1, 3)):
        assert pl_field(5, G, [[5] * G] * (planes - 1) + [[5] * (G - 1) + [x]])[2] == (G << 4 | t)
    assert (str(INT32_MAX) + "\n").encode() in text and (str(M + 1) + "\n").encode() in text


@pytest.mark.parametrize("with_gp,with_cov", [(False, False), (False, True), (True, False), (True, True)], ids=["pl", "covs-pl", "gp-pl", "covs-gp-pl"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 64])
def test_rows_are_exact(ctx, planes, haploid, with_gp, with_cov):
    """33 records (two write tiles): G = 0, 1, 15 (the long desc) and A = 16 among them; with and without the mask"""
    alleles = ([0, 1, 2, 15, 16, 3, 2] if haploid else [0, 1, 2, 5, 16, 3, 2]) * 5
    case = _case(planes, alleles[:33], haploid, seed=planes + 2 * haploid + 4 * with_gp + 8 * with_cov)
    keys = (1, 127, 128, 32768, 200) if planes == 1 else (1, 2, 3, 4, 5)
    for min_gq in (None, 50):
        text, _ = _both(ctx, case, haploid, keys, with_gp, with_cov, min_gq, shifts=(1, 15) if min_gq else (0, 7))
        if min_gq:
            assert (b"\t.:" in text) if haploid else (b"\t./.:" in text)


def test_the_row_without_its_pl_is_the_masked_row(ctx):
    g1, g2, gq, cov, vao, probs, vgo, status, pl = case = _case(5, [2, 3, 1, 2] * 8, False, seed=31)
    pl[pl == M] = 17
    for min_gq in (None, 40):
        got, off = ctx.format_calls_pl(g1, g2, gq, False, vao, vgo, pl, cov=cov, min_gq=min_gq)
        plain, poff = ctx.format_calls(g1, g2, gq, False, cov=cov, var_allele_off=vao, min_gq=min_gq)
        for v in range(len(vao) - 1):
            cells = got[int(off[v]):int(off[v + 1])].decode()[1:-1].split("\t")
            assert "".join("\t" + c.rsplit(":", 1)[0] for c in cells) + "\n" == plain[int(poff[v]):int(poff[v + 1])].decode()


def test_no_record(ctx):
    z = np.zeros((2, 0), dtype=np.int32)
    one32, one64 = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    assert ctx.format_calls_pl(z, z, z, False, one32, one64, z)[0] == b""
    out, off = ctx.encode_calls_bcf_pl(z, z, z, False, (1, 2, 3, 4, 5), one32, one64, z)
    assert out == b"" and list(off) == [0]
    for bcf in (False, True):
        rc, need, out, guard, doff = _device_rows(ctx, bcf, (z, z, z, None, one32, None, one64, None, z), False, (1, 2, 3, 4, 5), False, False, None, 0)
        assert rc == 0 and need == 0 and list(doff) == [0] and (guard == 0xAA).all()


def test_rows_across_the_window_boundary(ctx):
    """diploid A = 16 at 64 planes: rows of tens of KB, each through several 16 KB windows of the write pass, values on the boundaries"""
    case = _case(64, [16, 2, 16], False, seed=9)
    text, bcf = _both(ctx, case, False, with_gp=False, shifts=(0, 15))
    assert len(text) > 3 * 16384 and len(bcf) > 16384


@pytest.mark.parametrize("bcf", [False, True], ids=["text", "bcf"])
def test_buffer_too_small(ctx, bcf):
    """the capacity one byte short and cutting inside a value: MG_ERR_LIMIT, the size right, row_off whole, nothing at or behind the capacity"""
    haploid, keys = False, (1, 2, 3, 4, 5)
    case = _case(3, [2, 3, 1, 5] * 9, haploid, seed=12)
    g1, g2, gq, cov, vao, probs, vgo, status, pl = case
    pl[:, int(vgo[20]):int(vgo[21])] = 123456
    want, want_off = _rows_bcf(case, haploid, keys, True, True, None) if bcf else _rows_text(case, haploid, True, True, None)
    n, P = len(vao) - 1, 3
    inside = int(want_off[21]) - 2                                                 # two bytes short of record 20's last value
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for cap in (inside, len(want) - 1):
        buf = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
        off = np.full(n + 1, 1 << 63, dtype=np.uint64)
        need = C.c_uint64(0)
        if bcf:
            call = lambda c: ctx._L.mg_encode_calls_bcf(ctx.h, C.byref(Cells(n, P, int(haploid), p(g1), p(g2), p(gq), 0, 0, p(cov), p(vao), p(probs), p(vgo), p(status), p(pl), None,
                                                                          CELLS_GP | CELLS_PL)), C.byref(BcfKeys(*keys)), p(buf) if c else None, c, p(off), C.byref(need))
        else:
            call = lambda c: ctx._L.mg_format_calls(ctx.h, C.byref(Cells(n, P, int(haploid), p(g1), p(g2), p(gq), 0, 0, p(cov), p(vao), p(probs), p(vgo), p(status), p(pl), None,
                                                                      CELLS_GP | CELLS_PL)), p(buf) if c else None, c, p(off), C.byref(need))
        assert call(cap) == MG_ERR_LIMIT and need.value == len(want)
        assert np.array_equal(off, want_off)
        assert (buf[cap:] == 0xAA).all()
        assert buf[:cap].tobytes() == want[:cap]
        assert call(need.value) == 0 and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
        for shift in (0, 7):
            rc, dneed, out, guard, doff = _device_rows(ctx, bcf, case, haploid, keys, True, True, None, cap, guard=4096, shift=shift)
            assert rc == MG_ERR_LIMIT and dneed == len(want)
            assert np.array_equal(doff, want_off)
            assert out == want[:cap]
            assert (guard == 0xAA).all(), "bytes at or behind the capacity were written"
    with pytest.raises(MalvaError) as e:
        (ctx.encode_calls_bcf_pl(g1, g2, gq, haploid, keys, vao, vgo, pl, out_cap=len(want) - 1, probs=probs, status=status, cov=cov) if bcf else
         ctx.format_calls_pl(g1, g2, gq, haploid, vao, vgo, pl, text_cap=len(want) - 1, probs=probs, status=status, cov=cov))
    assert e.value.code == MG_ERR_LIMIT and e.value.needed == len(want) and np.array_equal(e.value.row_off, want_off)


def test_arguments(ctx):
    g = np.zeros((2, 2), dtype=np.int32)
    vao, vgo = np.array([0, 2, 4], dtype=np.uint32), np.array([0, 3, 6], dtype=np.uint64)
    probs, status, pl = np.zeros((2, 6)), np.zeros((2, 2), dtype=np.uint8), np.zeros((2, 6), dtype=np.int32)
    with pytest.raises(MalvaError, match="required"):
        ctx.format_calls_pl(g, g, g, False, None, vgo, pl)
    with pytest.raises(MalvaError, match="required"):
        ctx.encode_calls_bcf_pl(g, g, g, False, (1, 2, 3, 4, 5), vao, None, pl)
    with pytest.raises(MalvaError, match="NULL"):
        ctx.format_calls_pl(g, g, g, False, vao, vgo, None)
    with pytest.raises(MalvaError, match="go together"):
        ctx.format_calls_pl(g, g, g, False, vao, vgo, pl, probs=probs)
    with pytest.raises(MalvaError, match="go together"):
        ctx.encode_calls_bcf_pl(g, g, g, False, (1, 2, 3, 4, 5), vao, vgo, pl, status=status)
    with pytest.raises(MalvaError, match="dictionary"):
        ctx.encode_calls_bcf_pl(g, g, g, False, (1, 2, 3, 4, -5), vao, vgo, pl)
    ctx.encode_calls_bcf_pl(g, g, g, False, (1, 2, -3, -4, 5), vao, vgo, pl)         # the keys of fields that are not there are not read
    with pytest.raises(MalvaError, match="n_planes"):
        ctx.format_calls_pl(np.zeros((65, 2), dtype=np.int32), g, g, False, vao, vgo, pl)


# ---- the command line ---------------------------------------------------------------------------------------------------------

def _without_pl(text):
    """the merged file with the one header line, the FORMAT key and every cell's PL taken out -> (text, per record the cells' PL)"""
    out, pls = [], []
    for l in text.split("\n"):
        if l.startswith("##FORMAT=<ID=PL,"):
            continue
        if l and not l.startswith("#"):
            f = l.split("\t")
            assert f[8].endswith(":PL")
            pls.append([c.rsplit(":", 1)[1] for c in f[9:]])
            l = "\t".join(f[:8] + [f[8][:-3]] + [c.rsplit(":", 1)[0] for c in f[9:]])
        out.append(l)
    return "\n".join(out), pls


@pytest.mark.parametrize("mode", ["haploid", "diploid"])
def test_cli_pl_is_the_model_on_the_cells_own_covs(cohorts, tmp_path, mode):
    """-v --pl: every cell's PL is pl_model on that cell's own COVS; everything else is the file made without --pl.  And in BCF: ubcf and
    bcf decode to the text"""
    haploid = mode == "haploid"
    with_pl, without = str(tmp_path / "pl.vcf"), str(tmp_path / "plain.vcf")
    assert _run(cohorts, mode, ["-v", "--pl"], with_pl) == b"" and _run(cohorts, mode, ["-v"], without) == b""
    text = open(with_pl).read()
    head = [l for l in text.split("\n") if l.startswith("##")]
    at = [i for i, l in enumerate(head) if l.startswith("##FORMAT=<ID=PL,Number=G,Type=Integer,")]
    assert len(at) == 1 and head[at[0] - 1].startswith("##FORMAT=<ID=COVS,") and "prior-free" in head[at[0]] and "capped" in head[at[0]]
    stripped, pls = _without_pl(text)
    assert stripped == open(without).read()
    recs = _records(text)
    assert len(recs) > 100 and all(r[8] == "GT:GQ:COVS:PL" for r in recs)
    multi = capped = 0
    for r, pl in zip(recs, pls):
        for cell, got in zip(r[9:], pl):
            cov = [int(x) for x in cell.split(":")[2].split(",")]
            assert got == pl_text(pl_model.pl_cell(cov, 0.001, 200, haploid, 255)), (r[:5], cell)
            multi += len(cov) > 2
            capped += "255" in got.split(",")
    assert capped > 0 and (haploid or multi > 0)
    for fmt in ("ubcf", "bcf"):
        target = str(tmp_path / ("pl." + fmt))
        assert _run(cohorts, mode, ["-v", "--pl"], target, fmt) == b""
        data = open(target, "rb").read()
        lines = bcf_to_vcf(b"".join(raw for _, raw in bgzf_members(data)) if fmt == "bcf" else data)
        assert [l for l in lines if l.startswith("##FORMAT=<ID=PL,")]
        assert _records("\n".join(lines)) == recs
    assert sorted(os.listdir(tmp_path)) == ["pl.bcf", "pl.ubcf", "pl.vcf", "plain.vcf"]


def test_cli_gp_and_pl_and_the_cap_and_the_mask(cohorts, tmp_path):
    """--gp --pl: GT:GQ:GP:PL, the cells without their PL those of --gp alone, PL's header line behind GP's; --pl-cap 30 caps; --min-gq leaves PL in place;
    the whole also as BCF"""
    from test_gpu_bcf import _median_gq
    from test_gpu_gp import _gp_bits
    a, b, c, m = (str(tmp_path / f) for f in ("gp_pl.vcf", "gp.vcf", "cap.vcf", "mask.vcf"))
    _run(cohorts, "diploid", ["--gp", "--pl"], a)
    _run(cohorts, "diploid", ["--gp"], b)
    _run(cohorts, "diploid", ["--pl", "--pl-cap", "30"], c)
    text = open(a).read()
    head = [l for l in text.split("\n") if l.startswith("##")]
    at = [i for i, l in enumerate(head) if l.startswith("##FORMAT=<ID=PL,")]
    assert len(at) == 1 and head[at[0] - 1].startswith("##FORMAT=<ID=GP,")
    stripped, pls = _without_pl(text)
    assert stripped == open(b).read() and all(r[8] == "GT:GQ:GP:PL" for r in _records(text))
    capped, pls30 = _without_pl(open(c).read())
    assert all(r[8] == "GT:GQ" for r in _records(capped))
    n30 = 0
    for r255, r30 in zip(pls, pls30):
        for x, y in zip(r255, r30):
            assert y == ",".join(v if v == "." else str(min(int(v), 30)) for v in x.split(","))
            n30 += "30" in y.split(",") and x != y
    assert n30 > 0
    q = _median_gq(stripped)
    _run(cohorts, "diploid", ["--gp", "--pl", "--min-gq", str(q), "--site-tags"], m)
    masked = 0
    for ra, rm in zip(_records(text), _records(open(m).read())):
        for ca, cm in zip(ra[9:], rm[9:]):
            gt, gq, rest = ca.split(":", 2)
            if int(gq) < q:
                assert cm == "./.:%s:%s" % (gq, rest)
                masked += 1
            else:
                assert cm == ca
    assert masked > 0
    ub = str(tmp_path / "gp_pl.ubcf")
    _run(cohorts, "diploid", ["--gp", "--pl"], ub, "ubcf")
    binary = _records("\n".join(bcf_to_vcf(open(ub, "rb").read(), float_text=_gp_bits)))
    for rt, rb in zip(_records(text), binary):
        assert rt[:9] == rb[:9] and [x.rsplit(":", 1)[1] for x in rt[9:]] == [x.rsplit(":", 1)[1] for x in rb[9:]]


def test_cli_pl_does_not_depend_on_the_priors_or_the_grouping(cohorts, tmp_path):
    """the PL columns are those of the plain run under --cohort-priors --prior-iters 3, and under --prior-groups --cohort-group 2 (text and ubcf:
    the paste of the groups' blocks); the calls themselves differ, so the comparison is not vacuous"""
    plain, priors, groups, gub, pub = (str(tmp_path / f) for f in ("plain.vcf", "priors.vcf", "groups.vcf", "groups.ubcf", "priors.ubcf"))
    _run(cohorts, "diploid", ["--pl"], plain)
    _run(cohorts, "diploid", ["--pl", "--cohort-priors", "--prior-iters", "3"], priors)
    _run(cohorts, "diploid", ["--pl", "--cohort-priors", "--prior-iters", "3", "--prior-groups", "--cohort-group", "2"], groups)
    _run(cohorts, "diploid", ["--pl", "--cohort-priors", "--prior-iters", "3", "--prior-groups", "--cohort-group", "2"], gub, "ubcf")
    _run(cohorts, "diploid", ["--pl", "--cohort-priors", "--prior-iters", "3"], pub, "ubcf")
    base, pl0 = _without_pl(open(plain).read())
    other, pl1 = _without_pl(open(priors).read())
    assert pl0 == pl1 and len(pl0) > 100
    differ = sum(ca != cb for ra, rb in zip(_records(base), _records(other)) for ca, cb in zip(ra[9:], rb[9:]))
    assert differ > 0, "the priors changed no GT and no GQ: the comparison shows nothing"
    assert open(groups).read() == open(priors).read()
    assert open(gub, "rb").read() == open(pub, "rb").read()
    assert _records("\n".join(bcf_to_vcf(open(gub, "rb").read()))) == _records(open(priors).read())
    assert sorted(os.listdir(tmp_path)) == ["groups.ubcf", "groups.vcf", "plain.vcf", "priors.ubcf", "priors.vcf"]
