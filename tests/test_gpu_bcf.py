"""`call --cohort --merged --merged-format bcf|ubcf`: the multi-sample file as BCF2, its per-sample blocks made on the device
(mg_encode_calls_bcf).

The ABI is compared byte for byte with two restatements of the layout written here (struct, one value at a time; numpy, for the
sizes the first would take minutes for); the command line with the `--merged` VCF of the same run, through the BCF decoder of
tests/test_bcf_out_cpu.py.  Every comparison is exact."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

from malva_amd import Context, MalvaError, synth
from malva_amd.capi import BcfKeys, Cells
from test_bcf_out_cpu import bcf_to_vcf, bgzf_members, BGZF_EOF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
MG_ERR_LIMIT, MG_ERR_STATE = -5, -3
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
GT_EDGES = [62, 63, 16382, 16383, -1, (1 << 30) - 2, (1 << 30) - 1, INT_MAX]
VAL_EDGES = [-121, -120, 127, 128, -32761, -32760, 32767, 32768, INT_MIN + 8, INT_MAX]
COV_EDGES = VAL_EDGES + [1 << 31, (1 << 32) - 1]
ALLELES = [1, 2, 14, 15, 16, 128]
KEYS = [0, 127, 128, 32767, 32768]
PACK = {1: "<b", 2: "<h", 3: "<i"}
DTYPE = {1: "<i1", 2: "<i2", 3: "<i4"}


# ---- the encoders of the test -------------------------------------------------------------------------------------------------

def int_type(lo, hi):
    if lo >= -120 and hi <= 127:
        return 1
    if lo >= -32760 and hi <= 32767:
        return 2
    return 3


def typed_int(x):
    t = int_type(x, x)
    return bytes([0x10 | t]) + struct.pack(PACK[t], x)


def desc(n, t):
    return bytes([n << 4 | t]) if n < 15 else bytes([0xF0 | t]) + typed_int(n)


def gt_code(a, masked):
    return 0 if masked or a < 0 or a > (1 << 30) - 2 else (a + 1) << 1


def field(key, n, vals):
    """vals: the field's values over all planes, n per plane"""
    t = int_type(min(vals), max(vals)) if vals else 1
    return typed_int(key) + desc(n, t) + b"".join(struct.pack(PACK[t], x) for x in vals)


def encode_plain(g1, g2, gq, haploid, keys, cov=None, vao=None, min_gq=None):
    """-> (bytes, row_off), one struct.pack per value"""
    P, n = g1.shape
    rows = []
    for v in range(n):
        masked = [min_gq is not None and int(gq[p, v]) < min_gq for p in range(P)]
        codes = []
        for p in range(P):
            codes.append(gt_code(int(g1[p, v]), masked[p]))
            if not haploid:
                codes.append(gt_code(int(g2[p, v]), masked[p]))
        row = field(keys[0], 1 if haploid else 2, codes) + field(keys[1], 1, [int(gq[p, v]) for p in range(P)])
        if cov is not None:
            A = int(vao[v + 1]) - int(vao[v])
            row += field(keys[2], A, [int(np.int32(np.uint32(x))) for p in range(P) for x in cov[p, vao[v]:vao[v + 1]]])
        rows.append(row)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return b"".join(rows), off


def encode_numpy(g1, g2, gq, haploid, keys, cov=None, vao=None, min_gq=None):
    """the same bytes laid out with array arithmetic: the records are taken class by class, a class being the records whose rows
    have one shape (the three types and the allele count); the two are held against each other on every small case"""
    P, n = g1.shape
    q = gq.astype(np.int64).T                                                     # [n, P]
    masked = q < min_gq if min_gq is not None else np.zeros(q.shape, dtype=bool)

    def code(g):
        a = g.astype(np.int64).T
        return np.where(masked | (a < 0) | (a > (1 << 30) - 2), 0, (a + 1) << 1)
    codes = code(g1)[:, :, None] if haploid else np.stack([code(g1), code(g2)], axis=2)
    codes = codes.reshape(n, P * (1 if haploid else 2))

    def types(lo, hi):
        return np.where((lo >= -120) & (hi <= 127), 1, np.where((lo >= -32760) & (hi <= 32767), 2, 3))
    t_gt = types(codes.min(axis=1), codes.max(axis=1)) if n else np.zeros(0, dtype=np.int64)
    t_gq = types(q.min(axis=1), q.max(axis=1)) if n else np.zeros(0, dtype=np.int64)
    if cov is not None:
        cv = cov.astype(np.uint32).view(np.int32).astype(np.int64)                # [P, slots], the (int) cast
        A = (vao[1:].astype(np.int64) - vao[:-1].astype(np.int64))
        assert (A > 0).all()
        lo = np.minimum.reduceat(cv.min(axis=0), vao[:-1].astype(np.int64)) if n else np.zeros(0, dtype=np.int64)
        hi = np.maximum.reduceat(cv.max(axis=0), vao[:-1].astype(np.int64)) if n else np.zeros(0, dtype=np.int64)
        t_cov = types(lo, hi)
    else:
        A, t_cov = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    klass = ((t_gt * 4 + t_gq) * 4 + t_cov) * 1024 + A
    row_len = np.zeros(n, dtype=np.int64)
    mats = {}
    for k in np.unique(klass):
        idx = np.nonzero(klass == k)[0]
        tg, tq, tc, a = int(t_gt[idx[0]]), int(t_gq[idx[0]]), int(t_cov[idx[0]]), int(A[idx[0]])

        def part(key, per, t, vals):
            head = np.frombuffer(typed_int(key) + desc(per, t), dtype=np.uint8)
            return [np.broadcast_to(head, (len(idx), len(head))), np.ascontiguousarray(vals.astype(DTYPE[t])).view(np.uint8).reshape(len(idx), -1)]
        cols = part(keys[0], 1 if haploid else 2, tg, codes[idx]) + part(keys[1], 1, tq, q[idx])
        if cov is not None:
            slots = vao[:-1].astype(np.int64)[idx][:, None] + np.arange(a)[None, :]
            cols += part(keys[2], a, tc, cv[:, slots].transpose(1, 0, 2).reshape(len(idx), -1))
        mats[k] = (idx, np.concatenate(cols, axis=1))
        row_len[idx] = mats[k][1].shape[1]
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(row_len)
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    for idx, mat in mats.values():
        out[off[idx][:, None] + np.arange(mat.shape[1])[None, :]] = mat
    return out.tobytes(), off.astype(np.uint64)


def _case(planes, n, haploid, with_cov, seed, alleles=None):
    """numbers as a call gives them with the edge values strewn in, and every edge value once in one plane only -- the first or the
    last -- of a record whose other cells are small, so that a reduction that loses a lane shows"""
    rng = np.random.default_rng(seed)
    g1, g2 = (rng.integers(0, 3, size=(planes, n)).astype(np.int32) for _ in range(2))
    gq = rng.integers(0, 100, size=(planes, n)).astype(np.int32)
    for arr, edges in ((g1, GT_EDGES), (g2, GT_EDGES), (gq, VAL_EDGES)):
        pick = rng.random(arr.shape) < 0.02
        arr[pick] = np.array(edges, dtype=np.int64)[rng.integers(0, len(edges), size=int(pick.sum()))].astype(np.int32)
    if n:
        at = rng.permutation(n)
        j = 0
        for arr, edges in ((g1, GT_EDGES), (g2, GT_EDGES), (gq, VAL_EDGES)):
            for e in edges:
                for plane in (0, planes - 1):
                    v = at[j % n]
                    j += 1
                    if n > 3 * (len(GT_EDGES) * 2 + len(VAL_EDGES)) * 2:          # (room for a record of its own)
                        arr[:, v] = rng.integers(0, 3, size=planes)
                    arr[plane, v] = np.int64(e).astype(np.int32)
    if haploid:
        g2[:] = -1
    cov = vao = None
    if with_cov:
        al = np.array(alleles if alleles is not None else ALLELES, dtype=np.int64)
        A = al[np.arange(n) % len(al)]
        vao = np.zeros(n + 1, dtype=np.uint32)
        vao[1:] = np.cumsum(A)
        slots = int(vao[-1])
        cov = rng.integers(0, 100, size=(planes, slots)).astype(np.uint32)
        pick = rng.random(cov.shape) < 0.002
        cov[pick] = np.array(COV_EDGES, dtype=np.int64)[rng.integers(0, len(COV_EDGES), size=int(pick.sum()))].astype(np.uint32)
        if n:
            recs = rng.permutation(n)
            for j, e in enumerate(COV_EDGES * 2):
                v = recs[j % n]
                plane = 0 if j < len(COV_EDGES) else planes - 1
                if n > 2 * len(COV_EDGES):
                    cov[:, vao[v]:vao[v + 1]] = rng.integers(0, 100, size=(planes, int(A[v])))
                cov[plane, vao[v] + (int(A[v]) - 1 if j % 2 else 0)] = np.int64(e).astype(np.uint32)
    return g1, g2, gq, cov, vao


# ---- the ABI ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def test_bcf_stats_before_the_first_call():
    with Context(35, 43, 1 << 20) as c:
        with pytest.raises(MalvaError) as e:
            c.bcf_stats()
        assert e.value.code == MG_ERR_STATE
        g = np.zeros((2, 3), dtype=np.int32)
        c.encode_calls_bcf(g, g, g, False, (1, 2, 3))
        ms = c.bcf_stats()
        assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)


def test_bcf_stats_after_an_empty_call():
    with Context(35, 43, 1 << 20) as c:
        g = np.zeros((2, 0), dtype=np.int32)
        out, off = c.encode_calls_bcf(g, g, g, False, (1, 2, 3))                  # no record: the call still counts as one
        assert out == b"" and list(off) == [0]
        ms = c.bcf_stats()
        assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)


def _device_form(ctx, g1, g2, gq, haploid, keys, cov, vao, min_gq, cap, guard=64, shift=0):
    """-> (rc, need, bytes [cap], guard bytes, row_off); the buffer starts `shift` bytes into its allocation"""
    dev = torch.device("cuda", 0)
    P, n = g1.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)).view(np.int32)).to(dev)
    d1, d2, dq, dc, dv = t(g1), t(g2), t(gq), t(cov), t(vao)
    out = torch.full((shift + cap + guard,), 0xAA, dtype=torch.uint8, device=dev)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ptr = lambda x: 0 if x is None else x.data_ptr()
    rc, need = ctx.encode_calls_bcf_device(n, P, haploid, ptr(d1), ptr(d2), ptr(dq), ptr(dc), ptr(dv), keys, out.data_ptr() + shift if cap else 0, cap,
                                           off.data_ptr(), min_gq=min_gq)
    ctx.synchronize()
    h = out.cpu().numpy()
    assert (h[:shift] == 0xAA).all(), "bytes in front of the buffer were written"
    return rc, need, h[shift:shift + cap].tobytes(), h[shift + cap:], off.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 257])
@pytest.mark.parametrize("with_cov", [False, True], ids=["gt-gq", "gt-gq-covs"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 2, 63, 64])
def test_encode_calls_bcf_is_exact(ctx, planes, haploid, with_cov, n):
    g1, g2, gq, cov, vao = _case(planes, n, haploid, with_cov, seed=planes * 1000 + n + 2 * haploid + with_cov)
    keys = tuple(KEYS[(planes + n + i) % len(KEYS)] for i in range(3))
    for min_gq in (None, 50):
        want, want_off = encode_numpy(g1, g2, gq, haploid, keys, cov, vao, min_gq)
        plain, plain_off = encode_plain(g1, g2, gq, haploid, keys, cov, vao, min_gq)
        assert plain == want and np.array_equal(plain_off, want_off), "the two encoders of the test disagree"
        got, off = ctx.encode_calls_bcf(g1, g2, gq, haploid, keys, cov, vao, min_gq=min_gq)
        assert np.array_equal(off, want_off)
        assert len(got) == len(want)
        assert got == want
        ms = ctx.bcf_stats()
        assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)
        for shift in (0, 5):                                                      # the device form; once into a buffer that is not 16-byte aligned
            rc, need, out, guard, doff = _device_form(ctx, g1, g2, gq, haploid, keys, cov, vao, min_gq, len(want), shift=shift)
            assert rc == 0 and need == len(want)
            assert np.array_equal(doff, want_off)
            assert out == want
            assert (guard == 0xAA).all()


@pytest.mark.parametrize("key", KEYS)
def test_every_key_width_and_every_type_step(ctx, key):
    """one record per edge value, the value in the first or the last plane only: the type of the field is the restatement's"""
    planes = 5
    for edges, which in ((GT_EDGES, 0), (VAL_EDGES, 1), (COV_EDGES, 2)):
        for plane in (0, planes - 1):
            n = len(edges)
            g1 = np.ones((planes, n), dtype=np.int32)
            g2 = np.zeros((planes, n), dtype=np.int32)
            gq = np.full((planes, n), 7, dtype=np.int32)
            vao = (np.arange(n + 1) * 2).astype(np.uint32)
            cov = np.full((planes, 2 * n), 3, dtype=np.uint32)
            target = (g2, gq, cov)[which]
            for j, e in enumerate(edges):
                target[plane, 2 * j + 1 if which == 2 else j] = np.int64(e).astype(np.uint32 if which == 2 else np.int32)
            keys = (key, KEYS[(KEYS.index(key) + 1) % len(KEYS)], KEYS[(KEYS.index(key) + 2) % len(KEYS)])
            want, want_off = encode_plain(g1, g2, gq, False, keys, cov, vao)
            got, off = ctx.encode_calls_bcf(g1, g2, gq, False, keys, cov, vao)
            assert np.array_equal(off, want_off) and got == want, (which, plane)
    # what the edges must give, spelt out once: GT index 62 is int8's last, 63 int16's first, ...
    row = lambda a: ctx.encode_calls_bcf(np.array([[0], [a]], dtype=np.int32), None, np.zeros((2, 1), dtype=np.int32), True, (1, 2, 0))[0]
    assert row(62) == bytes([0x11, 1, 0x11, 2, 126, 0x11, 2, 0x11, 0, 0])
    assert row(63) == bytes([0x11, 1, 0x12, 2, 0, 128, 0, 0x11, 2, 0x11, 0, 0])
    assert row(16383) == bytes([0x11, 1, 0x13, 2, 0, 0, 0, 0, 128, 0, 0, 0x11, 2, 0x11, 0, 0])
    assert row(-1) == row(1 << 30) == row(INT_MAX) == bytes([0x11, 1, 0x11, 2, 0, 0x11, 2, 0x11, 0, 0])
    assert row((1 << 30) - 2)[2:11] == bytes([0x13, 2, 0, 0, 0]) + struct.pack("<i", INT_MAX - 1)


def test_encode_calls_bcf_across_the_scan_tiles(ctx):
    """about 2e5 records x 3 planes: the offsets cross the scan's tiles and the rows many write tiles"""
    planes, n = 3, 200_003
    g1, g2, gq, cov, vao = _case(planes, n, False, True, seed=5, alleles=[1, 2, 3, 16])
    keys = (3, 128, 32768)
    want, want_off = encode_numpy(g1, g2, gq, False, keys, cov, vao, 40)
    got, off = ctx.encode_calls_bcf(g1, g2, gq, False, keys, cov, vao, min_gq=40)
    assert np.array_equal(off, want_off)
    assert got == want
    rc, need, out, guard, doff = _device_form(ctx, g1, g2, gq, False, keys, cov, vao, 40, len(want), shift=3)
    assert rc == 0 and need == len(want) and np.array_equal(doff, want_off) and out == want and (guard == 0xAA).all()


@pytest.mark.parametrize("with_cov", [False, True], ids=["gt-gq", "gt-gq-covs"])
@pytest.mark.parametrize("planes,n", [(1, 1), (3, 257), (64, 300)])
def test_buffer_too_small(ctx, planes, n, with_cov):
    """out_cap 0, in the middle of a row, and one byte short: MG_ERR_LIMIT with the exact size, row_off valid, nothing at or behind
    out_cap touched, and the call with the size it reported succeeds -- host form and device form"""
    haploid = planes == 3
    keys = (1, 2, 3)
    g1, g2, gq, cov, vao = _case(planes, n, haploid, with_cov, seed=77 + planes)
    want, want_off = encode_numpy(g1, g2, gq, haploid, keys, cov, vao)
    middle = int(want_off[n // 2]) + (int(want_off[n // 2 + 1]) - int(want_off[n // 2])) // 2
    assert int(want_off[n // 2]) < middle < int(want_off[n // 2 + 1])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for cap in (0, middle, len(want) - 1):
        buf = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
        off = np.full(n + 1, 1 << 63, dtype=np.uint64)
        need = C.c_uint64(0)
        call = lambda cap_: ctx._L.mg_encode_calls_bcf(ctx.h, C.byref(Cells(n, planes, int(haploid), p(g1), p(g2), p(gq), 0, 0, p(cov), p(vao))), C.byref(BcfKeys(*keys)),
                                                       p(buf) if cap_ else None, cap_, p(off), C.byref(need))
        assert call(cap) == MG_ERR_LIMIT and need.value == len(want)
        assert np.array_equal(off, want_off)
        assert (buf[cap:] == 0xAA).all()
        assert buf[:cap].tobytes() == want[:cap]
        assert call(need.value) == 0 and need.value == len(want) and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
        for shift in (0, 7):
            rc, dneed, out, guard, doff = _device_form(ctx, g1, g2, gq, haploid, keys, cov, vao, None, cap, guard=4096, shift=shift)
            assert rc == MG_ERR_LIMIT and dneed == len(want)
            assert np.array_equal(doff, want_off)
            assert out == want[:cap]
            assert (guard == 0xAA).all(), "bytes behind out_cap were written"
            rc, dneed, out, guard, doff = _device_form(ctx, g1, g2, gq, haploid, keys, cov, vao, None, dneed, shift=shift)
            assert rc == 0 and out == want and (guard == 0xAA).all()
    with pytest.raises(MalvaError) as e:                                          # the binding hands the size and the offsets on
        ctx.encode_calls_bcf(g1, g2, gq, haploid, keys, cov, vao, out_cap=len(want) - 1)
    assert e.value.code == MG_ERR_LIMIT and e.value.needed == len(want) and np.array_equal(e.value.row_off, want_off)


def test_encode_calls_bcf_arguments(ctx):
    g = np.zeros((65, 2), dtype=np.int32)
    with pytest.raises(MalvaError, match="n_planes"):
        ctx.encode_calls_bcf(g, g, g, False, (1, 2, 3))
    g = np.zeros((2, 2), dtype=np.int32)
    with pytest.raises(MalvaError, match="go together"):
        ctx.encode_calls_bcf(g, g, g, False, (1, 2, 3), cov=np.zeros((2, 2), dtype=np.uint32))
    with pytest.raises(MalvaError, match="dictionary"):
        ctx.encode_calls_bcf(g, g, g, False, (-1, 2, 3))
    out, off = ctx.encode_calls_bcf(g, None, g, True, (1, 2, 3))                  # haploid: gt2 is not read
    assert out == bytes([0x11, 1, 0x11, 2, 2, 0x11, 2, 0x11, 0, 0]) * 2 and list(off) == [0, 10, 20]


# ---- the command line ---------------------------------------------------------------------------------------------------------

def _cli(args, env=None, binary=False):
    r = subprocess.run([BIN] + args, capture_output=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout if binary else r.stdout.decode()


def _sample_table(base, s, deep):
    """table of sample s (tests/test_gpu_cohort.py: two thirds of the base table's rows, another third for every s); counts of 1 .. 60,
    of 150 .. 249 for the deep sample: its coverages leave int8 where the others' stay inside"""
    hi, lo, cnt = base
    keep = (np.arange(len(hi)) + s) % 3 != 0
    c = cnt[keep].astype(np.uint64) * np.uint64(2 * s + 1) + np.uint64(7 * s)
    c = (150 + c % np.uint64(100) if deep else 1 + c % np.uint64(60)).astype(np.uint32)
    return np.ascontiguousarray(hi[keep]), np.ascontiguousarray(lo[keep]), c


K, REF_K, N_SAMPLES, DEEP = 35, 43, 5, 4


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """the diploid panel of indel / MNP clusters of tests/test_gpu_merged.py::test_cli_merged_on_general_blocks (multi-allelic records,
    no ##contig line in its header) and five samples, the last of them deep; indexed once diploid and, on a copy, once haploid"""
    data = tmp_path_factory.mktemp("bcf")
    panel = synth.indel_panel(1_500, seed=21, n_samples=70)
    base = synth.flat_kmer_table(panel, 60_000, K, REF_K, seed=5, max_records=1_200)
    out = {}
    for mode, flags in (("diploid", []), ("haploid", ["-1"])):
        d = data / mode
        d.mkdir()
        prefix = str(d / "p")
        synth.write_vcf_fasta(panel, prefix)
        lines = open(prefix + ".vcf").readlines()                                 # (the case is a header without ##contig lines)
        assert any(l.startswith("##contig") for l in lines)
        with open(prefix + ".vcf", "w") as fh:
            fh.writelines(l for l in lines if not l.startswith("##contig"))
        names = []
        for s in range(N_SAMPLES):
            hi, lo, cnt = _sample_table(base, s, s == DEEP)
            rows = synth.unpack_ascii(hi, lo, REF_K)
            with open(str(d / ("s%d.txt" % s)), "w") as fh:
                for r, c in zip(rows, cnt):
                    fh.write("%s\t%d\n" % (bytes(r[:REF_K]).decode(), int(c)))
            names.append("s%d" % s)
        (d / "cohort.tsv").write_text("".join("%s\t%s\n" % (n, n) for n in names))
        common = flags + ["-k", str(K), "-r", str(REF_K), "-b", "1", prefix + ".fa", prefix + ".vcf"]
        env = dict(os.environ, MALVA_GENO_BF_BITS=str(1 << 26), MALVA_GENO_BATCH="400")
        _cli(["index"] + common + [str(d / "s0")], env=env)
        out[mode] = (d, common, env, names)
    return out


def _run(cohort, mode, opts, target, fmt=None, group=(), env=None):
    d, common, env0, names = cohort[mode]
    return _cli(["call", "--cohort"] + list(opts) + list(group) + ["--merged", target] + ([] if fmt is None else ["--merged-format", fmt]) + common + [str(d / "cohort.tsv")],
                env=dict(env0, **(env or {})), binary=True)


def _af_text(key, bits):
    """AF as the text prints it, from the float the binary holds: the q (millionths) whose float32 it is, bit for bit"""
    if bits == 0x7F800001:
        return "."
    if key != "AF":
        return "%g" % struct.unpack("<f", struct.pack("<I", bits))[0]
    q = int(round(float(np.array([bits], dtype=np.uint32).view(np.float32)[0]) * 1e6))
    assert np.float32(int(q) / 1e6).view(np.uint32) == bits, "AF %08x is not the float32 of q / 1e6" % bits
    return "0" if q == 0 else "1" if q == 1000000 else ("0.%06d" % q).rstrip("0")


def _same_but_contigs(bcf_lines, vcf_text, fa):
    """the decoded BCF is the VCF line by line, but for the ##contig lines added in front of the ##INFO / #CHROM additions"""
    want = vcf_text.split("\n")
    assert want[-1] == ""
    want = want[:-1]
    added = [l for l in bcf_lines if l.startswith("##contig=")]
    seqs, name = [], None
    for line in open(fa):
        if line.startswith(">"):
            seqs.append([line[1:].split()[0], 0])
        else:
            seqs[-1][1] += len(line.strip())
    assert added == ["##contig=<ID=%s,length=%d>" % (n, l) for n, l in seqs] and len(added) >= 1
    at = bcf_lines.index(added[0])
    assert bcf_lines[at:at + len(added)] == added
    rest = bcf_lines[at + len(added):]
    assert all(l.startswith("##INFO=<ID=A") or l.startswith("##INFO=<ID=NS") or not l.startswith("##") for l in rest)   # (AC / AN / AF / NS, #CHROM, records)
    got = bcf_lines[:at] + rest
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % i
    return [l for l in want if not l.startswith("#")]


def _median_gq(vcf_text):
    gqs = sorted({int(c.split(":")[1]) for l in vcf_text.split("\n") if l and not l.startswith("#") for c in l.split("\t")[9:]})
    assert len(gqs) >= 2
    return gqs[len(gqs) // 2]


@pytest.fixture(scope="module")
def plain_vcf(cohort, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plain") / "plain.vcf")
    assert _run(cohort, "diploid", [], out) == b""
    return open(out).read()


@pytest.mark.parametrize("tag", ["plain", "haploid", "verbose", "min-gq", "site-tags", "all"])
def test_cli_ubcf_decodes_to_the_merged_vcf(cohort, plain_vcf, tmp_path, tag):
    q = str(_median_gq(plain_vcf))
    mode = "haploid" if tag == "haploid" else "diploid"
    opts = {"plain": [], "haploid": [], "verbose": ["-v"], "min-gq": ["--min-gq", q], "site-tags": ["--site-tags"], "all": ["-v", "--min-gq", q, "--site-tags"]}[tag]
    vcf, ubcf = str(tmp_path / "m.vcf"), str(tmp_path / "m.ubcf")
    assert _run(cohort, mode, opts, vcf, "vcf") == b"" and _run(cohort, mode, opts, ubcf, "ubcf") == b""
    text = open(vcf).read()
    if tag == "plain":
        assert text == plain_vcf                                                   # --merged-format vcf is no option at all
    data = open(ubcf, "rb").read()
    assert data[:5] == b"BCF\x02\x02"
    recs = _same_but_contigs(bcf_to_vcf(data, float_text=_af_text), text, cohort[mode][1][-2])
    assert len(recs) > 1000 and any("," in r.split("\t")[4] for r in recs), "no multi-allelic record"
    cells = [c for r in recs for c in r.split("\t")[9:]]
    assert len(cells) == N_SAMPLES * len(recs)
    if "--min-gq" in opts:
        assert any(c.startswith("./.:") for c in cells) and any(not c.startswith("./.:") for c in cells)
    if "--site-tags" in opts:
        assert any(r.split("\t")[7].startswith("AC=") and "AF=0." in r.split("\t")[7] for r in recs)
    if "-v" in opts:
        assert all(r.split("\t")[8] == "GT:GQ:COVS" for r in recs)
    if tag == "haploid":
        assert all("/" not in c for c in cells) and any(not c.startswith("0:") for c in cells)
    assert sorted(os.listdir(tmp_path)) == ["m.ubcf", "m.vcf"]


def test_cli_bcf_is_the_ubcf_in_bgzf_members(cohort, tmp_path):
    opts = ["-v", "--site-tags"]
    for group in ([], ["--cohort-group", "2"]):
        tagged = "".join(group).strip("-")
        bcf, ubcf = str(tmp_path / ("m%s.bcf" % tagged)), str(tmp_path / ("m%s.ubcf" % tagged))
        _run(cohort, "diploid", opts, bcf, "bcf", group)
        _run(cohort, "diploid", opts, ubcf, "ubcf", group)
        members = bgzf_members(open(bcf, "rb").read())
        assert len(members) > 2 and all(len(m) <= 1 << 16 and len(raw) <= 0xFF00 for m, raw in members)
        assert members[-1][0] == BGZF_EOF and all(len(raw) for _, raw in members[:-1])
        assert b"".join(raw for _, raw in members) == open(ubcf, "rb").read()
    assert open(str(tmp_path / "m.ubcf"), "rb").read() == open(str(tmp_path / "mcohort-group2.ubcf"), "rb").read()
    # stdout
    assert _run(cohort, "diploid", opts, "-", "ubcf", env={"TMPDIR": str(tmp_path)}) == open(str(tmp_path / "m.ubcf"), "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["m.bcf", "m.ubcf", "mcohort-group2.bcf", "mcohort-group2.ubcf"]


def test_cli_ubcf_does_not_depend_on_the_grouping(cohort, tmp_path):
    """--cohort-group 1, 2 and all: one file, although a field's type differs between the groups of some record (the deep sample's
    coverages); once more in batches of 7 records"""
    opts, files = ["-v", "--site-tags"], []
    for batch, group in (("400", []), ("400", ["--cohort-group", "1"]), ("400", ["--cohort-group", "2"]), ("7", ["--cohort-group", "2"])):
        d = tmp_path / ("".join(group).replace("-", "") + batch)
        d.mkdir()
        assert _run(cohort, "diploid", opts, str(d / "m.ubcf"), "ubcf", group, env={"MALVA_GENO_BATCH": batch}) == b""
        assert os.listdir(d) == ["m.ubcf"], "left beside the output"
        files.append(open(str(d / "m.ubcf"), "rb").read())
    assert len(set(files)) == 1, "the file depends on the grouping or the batching"
    recs = [l for l in bcf_to_vcf(files[0], float_text=_af_text) if not l.startswith("#")]
    mixed = 0
    for r in recs:
        covs = [[int(x) for x in c.split(":")[2].split(",")] for c in r.split("\t")[9:]]
        types = {int_type(min(sum(covs[a:a + 2], [])), max(sum(covs[a:a + 2], []))) for a in range(0, N_SAMPLES, 2)}
        mixed += len(types) > 1
    assert mixed > 0, "no record whose COVS type differs between the groups of two"
    d, common, env0, names = cohort["diploid"]
    assert not [f for f in os.listdir(d) if f.endswith(".part")]


def test_cli_the_products_own_reader_reads_the_bcf(cohort, tmp_path):
    """dump-kmers with the .bcf as the panel prints what it prints with the merged .vcf as the panel"""
    d, common, env0, names = cohort["diploid"]
    vcf, bcf, ubcf = str(tmp_path / "m.vcf"), str(tmp_path / "m.bcf"), str(tmp_path / "m.ubcf")
    for target, fmt in ((vcf, None), (bcf, "bcf"), (ubcf, "ubcf")):
        _run(cohort, "diploid", ["--site-tags"], target, fmt)
    dump = lambda panel: _cli(["dump-kmers"] + common[:-1] + [panel, "all"], env=env0)
    want = dump(vcf)
    assert want.count("VAR ") > 1000
    assert dump(bcf) == want and dump(ubcf) == want


def test_cli_out_dir_beside_the_bcf(cohort, tmp_path):
    """-o together with --merged-format bcf: the per-sample files are those of a run without it"""
    _run(cohort, "diploid", ["-o", str(tmp_path / "a")], str(tmp_path / "a.vcf"))
    for group in ([], ["--cohort-group", "2"]):
        out = tmp_path / ("b" + "".join(group).strip("-"))
        _run(cohort, "diploid", ["-o", str(out)], str(out) + ".bcf", "bcf", group)
        assert sorted(os.listdir(out)) == sorted(os.listdir(tmp_path / "a")) == ["s%d.vcf" % s for s in range(N_SAMPLES)]
        for f in os.listdir(out):
            assert open(str(out / f)).read() == open(str(tmp_path / "a" / f)).read(), f
    assert sorted(os.listdir(tmp_path)) == ["a", "a.vcf", "b", "b.bcf", "bcohort-group2", "bcohort-group2.bcf"]
