"""`call --cohort --merged --min-gq Q --site-tags`: a GQ mask on the sample columns and AC / AN / AF / NS in INFO, both made on the
device (mg_format_calls under a mask, mg_site_counts, mg_format_site_info).

The ABI is compared with numpy counts and with the rules restated in tests/test_site_tags_cpu.py; the command line with that
restatement applied to the plain merged file, which tests/test_gpu_merged.py pins.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from malva_amd import Context, MalvaError, synth
from malva_amd.capi import Cells
from test_gpu_merged import COMMON, _case, _cli, _no_leftovers, _singles, _split, format_plain, haploid_cohort  # noqa: F401 (the fixture)
from test_gpu_bcf import _case as _bcf_case, encode_plain
from test_site_tags_cpu import info_text

pytestmark = pytest.mark.gpu
MG_ERR_LIMIT, MG_ERR_STATE = -5, -3
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
ALLELES = np.array([1, 2, 3, 9, 100, 2, 2, 127, 0, 3], dtype=np.int64)             # records of these sizes, mixed
STRAY = np.array([-1, INT_MIN, INT_MAX, 127, 128, 1 << 20, 100, 9, 3, 2], dtype=np.int64)  # indices most records do not have
GUARD = 0xAAAAAAAA


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


# ---- the ABI: counts --------------------------------------------------------------------------------------------------------

def _counts_case(planes, n, seed):
    rng = np.random.default_rng(seed)
    A = ALLELES[rng.integers(0, len(ALLELES), size=n)]
    if n:
        A[:min(n, len(ALLELES))] = ALLELES[:min(n, len(ALLELES))]
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)

    def draw():
        g = (rng.random((planes, n)) * np.maximum(A, 1)[None, :]).astype(np.int64)  # inside the record (A = 0: 0, which is outside)
        stray = rng.random((planes, n)) < 0.03
        g[stray] = STRAY[rng.integers(0, len(STRAY), size=int(stray.sum()))]
        return g.astype(np.int32)
    g1, g2 = draw(), draw()
    gq = rng.integers(0, 60, size=(planes, n)).astype(np.int32)
    return g1, g2, gq, vao


def counts_numpy(g1, g2, gq, haploid, vao, min_gq):
    P, n = g1.shape
    called = np.ones((P, n), dtype=bool) if min_gq is None else gq >= min_gq
    A = np.diff(vao.astype(np.int64))
    ac = np.zeros(int(vao[-1]), dtype=np.int64)
    for g in ([g1] if haploid else [g1, g2]):
        g = g.astype(np.int64)
        ok = called & (g >= 0) & (g < A[None, :])
        ac += np.bincount((vao[:-1].astype(np.int64)[None, :] + g)[ok], minlength=ac.size)
    return ac.astype(np.uint32), called.sum(axis=0).astype(np.uint32)


def _counts_device_form(ctx, g1, g2, gq, haploid, vao, min_gq, accumulate=False, start=None, pad=256):
    """-> (ac, ns) from the device form, whose outputs lie between guard words that must survive"""
    dev = torch.device("cuda", 0)
    P, n = g1.shape
    slots = int(vao[-1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)).view(np.int32)).to(dev)
    d1, d2, dq, dv = t(g1), t(g2), t(gq), t(vao)
    ac = np.full(slots + 2 * pad, GUARD, dtype=np.uint32)
    ns = np.full(n + 2 * pad, GUARD, dtype=np.uint32)
    if start is not None:
        ac[pad:pad + slots], ns[pad:pad + n] = start
    dac, dns = t(ac), t(ns)
    torch.cuda.synchronize()
    ctx._ck(ctx._L.mg_site_counts_device(ctx.h, n, P, int(haploid), d1.data_ptr(), 0 if haploid else d2.data_ptr(), dq.data_ptr() if min_gq is not None else 0,
                                         int(min_gq is not None), int(min_gq or 0), dv.data_ptr(), int(accumulate), dac.data_ptr() + 4 * pad, dns.data_ptr() + 4 * pad))
    ctx.synchronize()
    hac, hns = dac.cpu().numpy().view(np.uint32), dns.cpu().numpy().view(np.uint32)
    for h, m in ((hac, slots), (hns, n)):
        assert (h[:pad] == GUARD).all() and (h[pad + m:] == GUARD).all(), "words outside the output were written"
    return hac[pad:pad + slots], hns[pad:pad + n]


@pytest.mark.parametrize("n", [0, 1, 257, 100003])
@pytest.mark.parametrize("masked", [False, True], ids=["all-called", "masked"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 3, 16, 17, 64])
def test_site_counts_are_exact(ctx, planes, haploid, masked, n):
    g1, g2, gq, vao = _counts_case(planes, n, seed=planes * 1000 + n % 997 + 2 * haploid + masked)
    min_gq = 30 if masked else None
    want_ac, want_ns = counts_numpy(g1, g2, gq, haploid, vao, min_gq)
    if n >= 257:
        assert want_ac.any() and (want_ns > 0).any()
        assert not masked or ((want_ns < planes).any() and counts_numpy(g1, g2, gq, haploid, vao, None)[0].sum() > want_ac.sum())
        assert (np.diff(vao.astype(np.int64)) == 100).any() and (np.diff(vao.astype(np.int64)) == 127).any()
    ac, ns = ctx.site_counts(g1, None if haploid else g2, gq, haploid, vao, min_gq=min_gq)
    assert np.array_equal(ns, want_ns)
    assert np.array_equal(ac, want_ac)
    ms = ctx.site_stats()
    assert len(ms) == 2 and all(m >= 0 for m in ms)
    dac, dns = _counts_device_form(ctx, g1, g2, gq, haploid, vao, min_gq)
    assert np.array_equal(dns, want_ns) and np.array_equal(dac, want_ac)


@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("n", [1, 257, 20011])
def test_site_counts_accumulate_over_split_planes(ctx, n, haploid):
    """two accumulating calls over split planes = one call over all of them; 130 planes from three calls = the numpy total"""
    g1, g2, gq, vao = _counts_case(130, n, seed=5 + n + haploid)
    for min_gq in (None, 25):
        for total, cuts in ((17, (0, 9, 17)), (64, (0, 1, 64)), (130, (0, 64, 128, 130))):
            want = counts_numpy(g1[:total], g2[:total], gq[:total], haploid, vao, min_gq)
            if total <= 64:
                one = ctx.site_counts(g1[:total], g2[:total], gq[:total], haploid, vao, min_gq=min_gq)
                assert np.array_equal(one[0], want[0]) and np.array_equal(one[1], want[1])
            ac = ns = dev = None                                                   # (the first call overwrites: the device form, guard words)
            for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
                ac, ns = ctx.site_counts(g1[lo:hi], g2[lo:hi], gq[lo:hi], haploid, vao, min_gq=min_gq, ac=ac, ns=ns)
                dev = _counts_device_form(ctx, g1[lo:hi], g2[lo:hi], gq[lo:hi], haploid, vao, min_gq, accumulate=j > 0, start=dev)
            assert np.array_equal(ac, want[0]) and np.array_equal(ns, want[1])
            assert np.array_equal(dev[0], want[0]) and np.array_equal(dev[1], want[1])


def test_site_counts_arguments(ctx):
    g = np.zeros((65, 2), dtype=np.int32)
    with pytest.raises(MalvaError, match="n_planes"):
        ctx.site_counts(g, g, g, False, np.array([0, 2, 4], dtype=np.uint32))
    g = np.array([[1, 0], [1, 5]], dtype=np.int32)
    ac, ns = ctx.site_counts(g, None, None, True, np.array([0, 2, 4], dtype=np.uint32))     # haploid, no mask: gt2 and gq are not read
    assert list(ac) == [0, 2, 1, 0] and list(ns) == [2, 2]


# ---- the ABI: INFO text -----------------------------------------------------------------------------------------------------

def _info_case(planes, n, haploid, masked, seed):
    """counts as the count entry gives them, with rows whose AN is 0 and a few large numbers put in"""
    g1, g2, gq, vao = _counts_case(planes, n, seed)
    ac, ns = counts_numpy(g1, g2, gq, haploid, vao, 30 if masked else None)
    rng = np.random.default_rng(seed + 1)
    for v in rng.integers(0, max(n, 1), size=min(n, 1 + n // 50)):
        ac[vao[v]:vao[v + 1]] = 0                                                     # AN = 0: every AF is '.'
        ns[v] = 0
    for v in rng.integers(0, max(n, 1), size=min(n, 1 + n // 50)):
        big = rng.choice(np.array([1, 9, 10, 999999, 1000000, 1 << 31, (1 << 32) - 1, 2000001, 3], dtype=np.uint64), size=int(vao[v + 1] - vao[v]))
        ac[vao[v]:vao[v + 1]] = big.astype(np.uint32)
        ns[v] = np.uint32(rng.choice(np.array([0, 7, (1 << 32) - 1], dtype=np.uint64)))
    return ac, ns, vao


def info_rows(ac, ns, vao):
    rows = [info_text(ac[vao[v]:vao[v + 1]], int(ns[v])) for v in range(ns.size)]
    off = np.zeros(ns.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return "".join(rows).encode(), off


def _info_device_form(ctx, ac, ns, vao, cap, guard=64, shift=0):
    dev = torch.device("cuda", 0)
    n = ns.size
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)).view(np.int32)).to(dev)
    dac, dns, dv = t(ac), t(ns), t(vao)
    text = torch.full((shift + cap + guard,), 0xAA, dtype=torch.uint8, device=dev)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    need = C.c_uint64(0)
    rc = ctx._L.mg_format_site_info_device(ctx.h, n, dac.data_ptr(), dns.data_ptr(), dv.data_ptr(), text.data_ptr() + shift if cap else 0, cap, off.data_ptr(),
                                           C.byref(need))
    ctx.synchronize()
    h = text.cpu().numpy()
    assert (h[:shift] == 0xAA).all(), "bytes in front of the buffer were written"
    return rc, need.value, h[shift:shift + cap].tobytes(), h[shift + cap:], off.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n", [0, 1, 257, 100003])
@pytest.mark.parametrize("masked", [False, True], ids=["all-called", "masked"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 3, 16, 17, 64])
def test_format_site_info_is_exact(ctx, planes, haploid, masked, n):
    ac, ns, vao = _info_case(planes, n, haploid, masked, seed=planes * 1000 + n % 997 + 2 * haploid + masked)
    want, want_off = info_rows(ac, ns, vao)
    if n >= 257:
        assert want.startswith(b"AN=") and b"AF=." in want and b"4294967295" in want  # (record 0 has no ALT; rows with AN = 0; a large count)
    got, off = ctx.format_site_info(ac, ns, vao)
    assert np.array_equal(off, want_off)
    assert len(got) == len(want)
    assert got == want
    for shift in (0, 5):
        rc, need, text, guard, doff = _info_device_form(ctx, ac, ns, vao, len(want), shift=shift)
        assert rc == 0 and need == len(want)
        assert np.array_equal(doff, want_off)
        assert text == want
        assert (guard == 0xAA).all()


def test_format_site_info_hand_written(ctx):
    vao = np.array([0, 3, 5, 6, 6, 8, 10, 12, 14], dtype=np.uint32)
    ac = np.array([3, 1, 2, 0, 0, 5, 0, 4, 1, 1, 2, 1, 2000000, 1], dtype=np.uint32)
    ns = np.array([3, 0, 5, 2, 2, 1, 2, 4294967295], dtype=np.uint32)
    rows = [b"AC=1,2;AN=6;AF=0.166667,0.333333;NS=3", b"AC=0;AN=0;AF=.;NS=0", b"AN=5;NS=5", b"AN=0;NS=2", b"AC=4;AN=4;AF=1;NS=2", b"AC=1;AN=2;AF=0.5;NS=1",
            b"AC=1;AN=3;AF=0.333333;NS=2", b"AC=1;AN=2000001;AF=0;NS=4294967295"]
    assert [info_text(ac[vao[v]:vao[v + 1]], int(ns[v])).encode() for v in range(8)] == rows
    text, off = ctx.format_site_info(ac, ns, vao)
    assert [text[int(off[v]):int(off[v + 1])] for v in range(8)] == rows and int(off[8]) == len(text)


@pytest.mark.parametrize("planes,n", [(1, 1), (3, 257), (17, 5000), (64, 40000)])
def test_site_info_buffer_too_small(ctx, planes, n):
    """text_cap one byte short, and 0: MG_ERR_LIMIT with the exact size, row_off valid, nothing at or behind text_cap touched, and the
    call with the size it reported succeeds -- host form and device form"""
    ac, ns, vao = _info_case(planes, n, planes == 3, False, seed=91 + planes)
    want, want_off = info_rows(ac, ns, vao)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for cap in (len(want) - 1, 0):
        buf = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
        off = np.full(n + 1, 1 << 63, dtype=np.uint64)
        need = C.c_uint64(0)
        rc = ctx._L.mg_format_site_info(ctx.h, n, p(ac), p(ns), p(vao), p(buf) if cap else None, cap, p(off), C.byref(need))
        assert rc == MG_ERR_LIMIT and need.value == len(want)
        assert np.array_equal(off, want_off)
        assert (buf[cap:] == 0xAA).all()
        rc = ctx._L.mg_format_site_info(ctx.h, n, p(ac), p(ns), p(vao), p(buf), need.value, p(off), C.byref(need))
        assert rc == 0 and need.value == len(want) and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
        for shift in (0, 7):
            rc, dneed, text, guard, doff = _info_device_form(ctx, ac, ns, vao, cap, guard=4096, shift=shift)
            assert rc == MG_ERR_LIMIT and dneed == len(want)
            assert np.array_equal(doff, want_off)
            assert (guard == 0xAA).all(), "bytes behind text_cap were written"
            rc, dneed, text, guard, doff = _info_device_form(ctx, ac, ns, vao, dneed, shift=shift)
            assert rc == 0 and text == want and (guard == 0xAA).all()
    with pytest.raises(MalvaError) as e:
        ctx.format_site_info(ac, ns, vao, text_cap=len(want) - 1)
    assert e.value.code == MG_ERR_LIMIT and e.value.needed == len(want) and np.array_equal(e.value.row_off, want_off)


def _stats_ok(ms, k):
    return len(ms) == k and all(np.isfinite(m) and m >= 0 for m in ms)


def test_site_stats_before_the_first_call_and_after_empty_ones():
    g, none, vao = np.zeros((2, 0), dtype=np.int32), np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    with Context(35, 43, 1 << 20) as c:
        with pytest.raises(MalvaError) as e:
            c.site_stats()
        assert e.value.code == MG_ERR_STATE
        ac, ns = c.site_counts(g, g, g, False, vao)                               # no record: the call still counts as one
        assert ac.size == 0 and ns.size == 0
        assert _stats_ok(c.site_stats(), 2)
    with Context(35, 43, 1 << 20) as c:
        text, off = c.format_site_info(none, none, vao)
        assert text == b"" and list(off) == [0]
        assert _stats_ok(c.site_stats(), 2)


def test_site_stats_with_one_kind_run():
    """0 for the kind that has not run"""
    g1, g2, gq, vao = _counts_case(3, 33, seed=8)
    ac, ns = counts_numpy(g1, g2, gq, False, vao, None)
    with Context(35, 43, 1 << 20) as c:
        c.site_counts(g1, g2, gq, False, vao)
        ms = c.site_stats()
        assert _stats_ok(ms, 2) and ms[1] == 0
    with Context(35, 43, 1 << 20) as c:
        c.format_site_info(ac, ns, vao)
        ms = c.site_stats()
        assert _stats_ok(ms, 2) and ms[0] == 0


# ---- the ABI: the encoders beside each other ----------------------------------------------------------------------------------

def test_the_encoders_do_not_disturb_each_other():
    """one context, 3 planes x 33 records (a full write tile and a ragged one): text, BCF, counts, INFO and the text again, through the
    host forms; then through the device forms, every output held on the device until the last call has run and compared only then"""
    planes, n, keys, min_gq = 3, 33, (1, 128, 32768), 50
    g1, g2, gq, cov, vao = _bcf_case(planes, n, False, True, seed=33)
    want_text = format_plain(g1, g2, gq, False, cov, vao)
    want_bcf = encode_plain(g1, g2, gq, False, keys, cov, vao, min_gq)
    want_ac, want_ns = counts_numpy(g1, g2, gq, False, vao, min_gq)
    want_info = info_rows(want_ac, want_ns, vao)
    assert want_ac.any() and (want_ns < planes).any()

    def same(got, want):
        assert np.array_equal(got[1], want[1]) and got[0] == want[0]
    with Context(35, 43, 1 << 20) as c:
        same(c.format_calls(g1, g2, gq, False, cov, vao), want_text)
        same(c.encode_calls_bcf(g1, g2, gq, False, keys, cov, vao, min_gq=min_gq), want_bcf)
        ac, ns = c.site_counts(g1, g2, gq, False, vao, min_gq=min_gq)
        assert np.array_equal(ac, want_ac) and np.array_equal(ns, want_ns)
        same(c.format_site_info(ac, ns, vao), want_info)
        same(c.format_calls(g1, g2, gq, False, cov, vao), want_text)
        assert _stats_ok(c.format_stats(), 3) and _stats_ok(c.bcf_stats(), 3) and _stats_ok(c.site_stats(), 2)

        dev = torch.device("cuda", 0)
        d1, d2, dq, dc, dv = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (g1, g2, gq, cov, vao))
        dac = torch.full((want_ac.size,), -1, dtype=torch.int32, device=dev)
        dns = torch.full((n,), -1, dtype=torch.int32, device=dev)
        held = []                                                                 # (what, bytes on the device, offsets on the device, wanted)

        def rows(what, want, call):
            out = torch.full((len(want[0]) + 64,), 0xAA, dtype=torch.uint8, device=dev)
            off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            assert call(out.data_ptr(), len(want[0]), off.data_ptr()) == (0, len(want[0])), what
            held.append((what, out, off, want))
        v = C.c_void_p

        def info(d_text, cap, d_off):
            need = C.c_uint64(0)
            return c._L.mg_format_site_info_device(c.h, n, v(dac.data_ptr()), v(dns.data_ptr()), v(dv.data_ptr()), v(d_text), cap, v(d_off), C.byref(need)), need.value
        text = lambda d_text, cap, d_off: c.format_calls_device(n, planes, False, d1.data_ptr(), d2.data_ptr(), dq.data_ptr(), dc.data_ptr(), dv.data_ptr(), d_text, cap, d_off)
        rows("text", want_text, text)
        rows("bcf", want_bcf, lambda d_out, cap, d_off: c.encode_calls_bcf_device(n, planes, False, d1.data_ptr(), d2.data_ptr(), dq.data_ptr(), dc.data_ptr(), dv.data_ptr(),
                                                                                 keys, d_out, cap, d_off, min_gq=min_gq))
        c._ck(c._L.mg_site_counts_device(c.h, n, planes, 0, v(d1.data_ptr()), v(d2.data_ptr()), v(dq.data_ptr()), 1, min_gq, v(dv.data_ptr()), 0, v(dac.data_ptr()),
                                         v(dns.data_ptr())))
        rows("info", want_info, info)
        rows("text again", want_text, text)
        c.synchronize()
        assert np.array_equal(dac.cpu().numpy().view(np.uint32), want_ac) and np.array_equal(dns.cpu().numpy().view(np.uint32), want_ns)
        for what, out, off, want in held:
            h = out.cpu().numpy()
            assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1]), what
            assert h[:len(want[0])].tobytes() == want[0], what
            assert (h[len(want[0]):] == 0xAA).all(), what
        assert _stats_ok(c.format_stats(), 3) and _stats_ok(c.bcf_stats(), 3) and _stats_ok(c.site_stats(), 2)


# ---- the ABI: masked cells --------------------------------------------------------------------------------------------------

def format_masked(g1, g2, gq, haploid, min_gq, cov=None, vao=None):
    """format_plain of tests/test_gpu_merged.py with the genotype of a cell whose gq < min_gq printed as missing"""
    P, n = g1.shape
    rows = []
    for v in range(n):
        cells = []
        for p in range(P):
            if int(gq[p, v]) < min_gq:
                c = "." if haploid else "./."
            else:
                c = str(int(g1[p, v])) if haploid else "%d/%d" % (int(g1[p, v]), int(g2[p, v]))
            c += ":%d" % int(gq[p, v])
            if cov is not None:
                c += ":" + ",".join(str(int(np.int32(np.uint32(x)))) for x in cov[p, vao[v]:vao[v + 1]])
            cells.append("\t" + c)
        rows.append("".join(cells) + "\n")
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return "".join(rows).encode(), off


@pytest.mark.parametrize("with_cov", [False, True], ids=["gt-gq", "gt-gq-covs"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes,n", [(1, 1), (3, 257), (17, 300), (64, 257), (16, 3000)])
def test_format_calls_masked_is_exact(ctx, planes, n, haploid, with_cov):
    g1, g2, gq, cov, vao = _case(planes, n, haploid, with_cov, seed=31 + planes + n)
    for min_gq in (100, 0, INT_MAX, 1):
        want, want_off = format_masked(g1, g2, gq, haploid, min_gq, cov, vao)
        if n >= 257:
            assert (b"\t.:" in want) == haploid and (b"\t./.:" in want) != haploid and want != format_plain(g1, g2, gq, haploid, cov, vao)[0]
        got, off = ctx.format_calls(g1, g2, gq, haploid, cov, vao, min_gq=min_gq)
        assert np.array_equal(off, want_off) and got == want
    # a min_gq below every GQ: mg_format_calls byte for byte
    plain, plain_off = ctx.format_calls(g1, g2, gq, haploid, cov, vao)
    assert plain == format_plain(g1, g2, gq, haploid, cov, vao)[0]
    got, off = ctx.format_calls(g1, g2, gq, haploid, cov, vao, min_gq=INT_MIN)
    assert got == plain and np.array_equal(off, plain_off)
    # the buffer contract of the masked entry, device form: one byte short, guard bytes behind text_cap
    want, want_off = format_masked(g1, g2, gq, haploid, 100, cov, vao)
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    ptr = lambda x: 0 if x is None else x.data_ptr()
    d1, d2, dq, dc, dv = t(g1), t(g2), t(gq), t(cov), t(vao)
    for cap in (len(want) - 1, len(want)):
        text = torch.full((3 + cap + 4096,), 0xAA, dtype=torch.uint8, device=dev)
        doff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        need = C.c_uint64(0)
        rc = ctx._L.mg_format_calls_device(ctx.h, C.byref(Cells(n, planes, int(haploid), ptr(d1), ptr(d2), ptr(dq), 1, 100, ptr(dc), ptr(dv))), text.data_ptr() + 3, cap,
                                           doff.data_ptr(), C.byref(need))
        ctx.synchronize()
        h = text.cpu().numpy()
        assert rc == (0 if cap == len(want) else MG_ERR_LIMIT) and need.value == len(want)
        assert np.array_equal(doff.cpu().numpy().view(np.uint64), want_off)
        assert h[3:3 + cap].tobytes() == want[:cap] and (h[:3] == 0xAA).all() and (h[3 + cap:] == 0xAA).all()


# ---- the command line -------------------------------------------------------------------------------------------------------

INFO_LINES = {"AC": '##INFO=<ID=AC,Number=A,Type=Integer,Description="Allele count in called genotypes, for each ALT allele">',
              "AN": '##INFO=<ID=AN,Number=1,Type=Integer,Description="Total number of alleles in called genotypes">',
              "AF": '##INFO=<ID=AF,Number=A,Type=Float,Description="Allele frequency in called genotypes, for each ALT allele">',
              "NS": '##INFO=<ID=NS,Number=1,Type=Integer,Description="Number of samples with a called genotype">'}


def _cells(rec):
    """-> [(genotype text, gq, rest)] of a record line"""
    out = []
    for cell in rec.split("\t")[9:]:
        parts = cell.split(":")
        out.append((parts[0], int(parts[1]), parts[2:]))
    return out


def restate(plain, min_gq, tags):
    """the rules applied to the plain merged text (with -v: the plain -v merged text) -> the text the options must give, and per
    record (ac, an) for the checks that keep the comparison from being vacuous"""
    head, recs = _split(plain)
    if tags:
        declared = {l[len("##INFO=<ID="):].split(",")[0].rstrip(">") for l in head if l.startswith("##INFO=<ID=")}
        head = head[:-1] + [INFO_LINES[t] for t in ("AC", "AN", "AF", "NS") if t not in declared] + head[-1:]
    out, counts, n_masked, n_called = [], [], 0, 0
    for rec in recs:
        cols = rec.split("\t")
        assert cols[7] == "."
        ac = [0] * (1 + (len(cols[4].split(",")) if cols[4] != "." else 0))
        ns = 0
        cells = []
        for gt, gq, rest in _cells(rec):
            if min_gq is not None and gq < min_gq:
                gt = "./." if "/" in gt else "."
                n_masked += 1
            else:
                n_called += 1
                ns += 1
                for a in gt.split("/"):
                    assert 0 <= int(a) < len(ac)
                    ac[int(a)] += 1
            cells.append(":".join([gt, str(gq)] + rest))
        counts.append((ac, sum(ac)))
        out.append("\t".join(cols[:7] + [info_text(ac, ns) if tags else "."] + [cols[8]] + cells))
    return "\n".join(head + out) + "\n", counts, n_masked, n_called


def _median_gq(plain):
    gqs = sorted({gq for rec in _split(plain)[1] for _, gq, _ in _cells(rec)})
    assert len(gqs) >= 2, "the cohort's cells carry one GQ only: %s" % gqs
    return gqs[len(gqs) // 2]


def _check_runs(run, plains, singles, names, groups, tmp_path):
    """run(opts, group, target, env=None) -> stdout of `call --cohort --merged target`; plains / singles: {verbose: text(s)}"""
    q = _median_gq(plains[False])
    assert q == _median_gq(plains[True])
    for tag, flags, verbose in (("gq", ["--min-gq", str(q)], False), ("tags", ["--site-tags"], False), ("both", ["--min-gq", str(q), "--site-tags"], False),
                                ("vboth", ["-v", "--min-gq", str(q), "--site-tags"], True)):
        masked, tags = "--min-gq" in flags, "--site-tags" in flags
        want, counts, n_masked, n_called = restate(plains[verbose], q if masked else None, tags)
        assert n_called and (n_masked > 0) == masked, "Q = %d masks %d cells and leaves %d" % (q, n_masked, n_called)
        if tags:
            assert any(0 < x < an for ac, an in counts for x in ac[1:]), "no record has 0 < AC < AN"
        assert want != plains[verbose]
        for group in groups:                                                       # one text, whatever the grouping
            d = tmp_path / (tag + "".join(group).strip("-"))
            d.mkdir()
            assert run(flags, group, str(d / "merged.vcf")) == ""
            _no_leftovers(d, ["merged.vcf"])
            assert open(str(d / "merged.vcf")).read() == want, "%s %s" % (flags, group)
        for group in (groups[0], groups[-1]):                                     # stdout, the groups' temporary files under $TMPDIR
            d = tmp_path / (tag + "stdout" + "".join(group).strip("-"))
            d.mkdir()
            assert run(flags, group, "-", env={"TMPDIR": str(d)}) == want
            _no_leftovers(d, [])
        for group in (groups[0], groups[-1]):                                     # -o alongside: the per-sample files are the single calls
            d = tmp_path / (tag + "both" + "".join(group).strip("-"))
            d.mkdir()
            assert run(flags + ["-o", str(d / "out")], group, str(d / "m.vcf")) == ""
            assert open(str(d / "m.vcf")).read() == want
            assert sorted(os.listdir(d / "out")) == sorted(n + ".vcf" for n in names)
            for n, single in zip(names, singles[verbose]):
                assert open(str(d / "out" / (n + ".vcf"))).read() == single, n
            _no_leftovers(d, ["m.vcf", "out"])


def test_cli_min_gq_and_site_tags_on_the_haploid_cohort(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    names = list(inputs)
    man = str(tmp / "cohort.tsv")
    _cli(["index"] + COMMON + [fa, vcf, fq])

    def run(opts, group, target, env=None):
        return _cli(["call"] + COMMON + opts + group + ["--cohort", "--merged", target, fa, vcf, man], env=dict(os.environ, **(env or {})))
    plains, singles = {}, {}
    for verbose in (False, True):
        out = str(tmp_path / ("plain%d.vcf" % verbose))
        run(["-v"] if verbose else [], [], out)
        plains[verbose] = open(out).read()
        os.remove(out)
        singles[verbose] = _singles(tmp, fa, vcf, inputs, ["-v"] if verbose else [])
    _check_runs(run, plains, singles, names, [[], ["--cohort-group", "1"], ["--cohort-group", "3"]], tmp_path)
    _no_leftovers(tmp, ["haploid.fq", "dump.txt", "sim1.fq", "sim2.fq", "keep.txt", "cohort.tsv"] + [f for f in os.listdir(tmp) if f.startswith("haploid.vcf.gz")])


def test_cli_min_gq_and_site_tags_on_general_blocks(tmp_path):
    """the diploid panel of tests/test_gpu_merged.py::test_cli_merged_on_general_blocks (multi-allelic records, a/b cells), in batches of
    7 records -- which the paste pass of a grouped run takes its counts in, too"""
    from test_gpu_cohort import _sample_table
    data = tmp_path / "data"
    data.mkdir()
    panel = synth.indel_panel(1_500, seed=21, n_samples=70)
    prefix = str(data / "p")
    synth.write_vcf_fasta(panel, prefix)
    k, ref_k = 35, 43
    names = []
    for s in range(3):
        hi, lo, cnt = _sample_table(synth.flat_kmer_table(panel, 60_000, k, ref_k, seed=5, max_records=1_200), s)
        rows = synth.unpack_ascii(hi, lo, ref_k)
        with open(str(data / ("s%d.txt" % s)), "w") as fh:
            for r, c in zip(rows, cnt):
                fh.write("%s\t%d\n" % (bytes(r[:ref_k]).decode(), int(c)))
        names.append("s%d" % s)
    (data / "cohort.tsv").write_text("".join("%s\t%s\n" % (n, n) for n in names))
    common = ["-k", str(k), "-r", str(ref_k), "-b", "1", prefix + ".fa", prefix + ".vcf"]
    env0 = dict(os.environ, MALVA_GENO_BF_BITS=str(1 << 26), MALVA_GENO_BATCH="7")
    _cli(["index"] + common + [str(data / "s0")], env=env0)

    def run(opts, group, target, env=None):
        return _cli(["call", "--cohort"] + opts + group + ["--merged", target] + common + [str(data / "cohort.tsv")], env=dict(env0, **(env or {})))
    plains, singles = {}, {}
    for verbose in (False, True):
        out = str(tmp_path / ("plain%d.vcf" % verbose))
        run(["-v"] if verbose else [], [], out)
        plains[verbose] = open(out).read()
        os.remove(out)
        singles[verbose] = [_cli(["call"] + (["-v"] if verbose else []) + common + [str(data / n)], env=env0) for n in names]
    assert any(len(r.split("\t")[4].split(",")) > 1 for r in _split(plains[False])[1]), "no multi-allelic record"
    _check_runs(run, plains, singles, names, [[], ["--cohort-group", "1"], ["--cohort-group", "2"]], tmp_path)
    assert not [f for f in os.listdir(data) if f.endswith(".part")]
