"""`call --cohort --merged --gp`: the genotype posteriors as the FORMAT field GP of the merged file, made on the device by
mg_format_calls (text) and mg_encode_calls_bcf (BCF2) under MG_CELLS_GP.

The expected bytes come from a restatement written here: Python's `"%.6f" % p` is correctly rounded on the exact binary value with
ties to even, numpy.float32(p) is IEEE round to nearest even.  The rest of a cell and of a BCF row -- everything that is not GP --
is what the tests of the entries without GP pin (test_gpu_merged.format_plain, test_gpu_bcf.encode_plain), taken from there.
Every comparison is exact but one: a value of the BCF against the same value of the text, whose bound is derived where it is used."""
import ctypes as C
import functools
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from malva_amd import Context, MalvaError, synth
from malva_amd.capi import CELLS_GP, BcfKeys, Cells
from test_bcf_out_cpu import bcf_to_vcf, bgzf_members
from test_gpu_bcf import desc, encode_plain, typed_int
from test_gpu_merged import format_plain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MG_ERR_LIMIT = -5
NORMAL = 0
F_MISSING, F_EOV = 0x7F800001, 0x7F800002
NAN, INF = float("nan"), float("inf")
PRINTABLE = [0.0, 1.0, math.nextafter(1.0, 0.0), 5e-324, 1e-40, 1e-7, 4.9999999e-7, 5e-7, 5.0000001e-7,
             math.nextafter(0.9999995, 0.0), 0.9999995, math.nextafter(0.9999995, 1.0), 1 / 128, 3 / 128, 127 / 128,
             2.0 ** -149, 2.0 ** -150, math.nextafter(2.0 ** -150, 1.0), 2.0 ** -126, math.nextafter(2.0 ** -126, 0.0), 0.1, 0.5, 1 / 3]
UNPRINTABLE = [NAN, -0.0, -0.25, math.nextafter(1.0, 2.0), INF, -INF, -NAN]
GARBAGE = [NAN, -7.5, 3e300, 0.123456]           # what a cell without a list may hold where its list would be: never read


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def printable(p):
    return struct.unpack("<Q", struct.pack("<d", p))[0] <= 0x3FF0000000000000     # sign clear and 0 <= p <= 1


def n_gt(A, haploid):
    return A if haploid else A * (A + 1) // 2


@functools.lru_cache(maxsize=None)
def vcf_order(A, haploid):
    """-> for every VCF index the place of that genotype in probs' order (a outer, c >= a inner)"""
    if haploid:
        return list(range(A))
    src = {}
    q = 0
    for a in range(A):
        for c in range(a, A):
            src[c * (c + 1) // 2 + a] = q
            q += 1
    return [src[g] for g in range(len(src))]


def gp_values(probs, vgo, vao, status, haploid, p, v):
    """the record's list of plane p in VCF order, or None where the cell has none"""
    if status[p, v] != NORMAL:
        return None
    A = int(vao[v + 1]) - int(vao[v])
    return [float(probs[p, int(vgo[v]) + s]) for s in vcf_order(A, haploid)]


def gp_text(vals):
    return "." if vals is None else ",".join("%.6f" % x if printable(x) else "." for x in vals)


def gp_floats(vals, G):
    if vals is None:
        return [F_MISSING] + [F_EOV] * (G - 1)
    with np.errstate(all="ignore"):
        return [int(np.float32(x).view(np.uint32)) if printable(x) else F_MISSING for x in vals]


def expect_text(g1, g2, gq, haploid, vao, probs, vgo, status, cov=None, min_gq=None):
    P, n = g1.shape
    if min_gq is not None:                                                         # a masked cell: the genotype alone goes missing
        base, off = format_plain(g1, g2, gq, haploid, cov, vao if cov is not None else None)
        rows = []
        for v in range(n):
            cells = base[int(off[v]):int(off[v + 1])].decode()[1:-1].split("\t")
            rows.append([("." if haploid else "./.") + c[c.index(":"):] if int(gq[p, v]) < min_gq else c for p, c in enumerate(cells)])
    else:
        base, off = format_plain(g1, g2, gq, haploid, cov, vao if cov is not None else None)
        rows = [base[int(off[v]):int(off[v + 1])].decode()[1:-1].split("\t") for v in range(n)]
    out = []
    for v in range(n):
        out.append(("".join("\t" + c + ":" + gp_text(gp_values(probs, vgo, vao, status, haploid, p, v)) for p, c in enumerate(rows[v])) + "\n").encode())
    o = np.zeros(n + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(r) for r in out])
    return b"".join(out), o


def expect_bcf(g1, g2, gq, haploid, keys, vao, probs, vgo, status, cov=None, min_gq=None):
    P, n = g1.shape
    base, off = encode_plain(g1, g2, gq, haploid, keys[:3], cov, vao, min_gq)
    out = []
    for v in range(n):
        G = n_gt(int(vao[v + 1]) - int(vao[v]), haploid)
        f = [x for p in range(P) for x in gp_floats(gp_values(probs, vgo, vao, status, haploid, p, v), G)]
        out.append(base[int(off[v]):int(off[v + 1])] + typed_int(keys[3]) + desc(G, 5) + struct.pack("<%dI" % len(f), *f))
    o = np.zeros(n + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(r) for r in out])
    return b"".join(out), o


def _case(planes, alleles, haploid, seed, with_cov=True, values=None):
    """one record per entry of `alleles`; the values of the lists are drawn from `values` (default: the edges and random ones)"""
    rng = np.random.default_rng(seed)
    n = len(alleles)
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(alleles)
    vgo = np.zeros(n + 1, dtype=np.uint64)
    vgo[1:] = np.cumsum([n_gt(a, haploid) for a in alleles])
    g1, g2 = (rng.integers(0, 3, size=(planes, n)).astype(np.int32) for _ in range(2))
    gq = rng.integers(0, 100, size=(planes, n)).astype(np.int32)
    cov = rng.integers(0, 300, size=(planes, int(vao[-1]))).astype(np.uint32) if with_cov else None
    pool = np.array(PRINTABLE + UNPRINTABLE if values is None else values, dtype=np.float64)
    probs = rng.random(size=(planes, int(vgo[-1])))
    edge = rng.random(size=probs.shape) < 0.4
    probs[edge] = pool[rng.integers(0, len(pool), size=int(edge.sum()))]
    status = np.where(rng.random(size=(planes, n)) < 0.2, rng.integers(1, 4, size=(planes, n)), 0).astype(np.uint8)
    for p in range(planes):                                                        # a cell without a list holds garbage there
        for v in np.nonzero(status[p])[0]:
            probs[p, int(vgo[v]):int(vgo[v + 1])] = np.resize(np.array(GARBAGE), int(vgo[v + 1]) - int(vgo[v]))
    return g1, g2, gq, cov, vao, probs, vgo, status


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def _device_form(ctx, bcf, case, haploid, keys, min_gq, cap, guard=64, shift=0):
    """-> (rc, need, bytes [cap], guard bytes, row_off); the buffer starts `shift` bytes into its allocation"""
    g1, g2, gq, cov, vao, probs, vgo, status = case
    dev = torch.device("cuda", 0)
    P, n = g1.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)).reshape(-1).view(np.uint8)).to(dev)
    d1, d2, dq, dc, dv, dp, dg, ds = (t(a) for a in (g1, g2, gq, cov, vao, probs, vgo, status))
    out = torch.full((shift + cap + guard,), 0xAA, dtype=torch.uint8, device=dev)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ptr = lambda x: 0 if x is None else x.data_ptr()
    dst = out.data_ptr() + shift if cap else 0
    if bcf:
        rc, need = ctx.encode_calls_bcf_gp_device(n, P, haploid, ptr(d1), ptr(d2), ptr(dq), ptr(dc), ptr(dv), ptr(dp), ptr(dg), ptr(ds), keys, dst, cap, off.data_ptr(),
                                                  min_gq=min_gq)
    else:
        rc, need = ctx.format_calls_gp_device(n, P, haploid, ptr(d1), ptr(d2), ptr(dq), ptr(dc), ptr(dv), ptr(dp), ptr(dg), ptr(ds), dst, cap, off.data_ptr(), min_gq=min_gq)
    ctx.synchronize()
    h = out.cpu().numpy()
    assert (h[:shift] == 0xAA).all(), "bytes in front of the buffer were written"
    return rc, need, h[shift:shift + cap].tobytes(), h[shift + cap:], off.cpu().numpy().view(np.uint64)


def _both(ctx, case, haploid, keys=(1, 2, 3, 4), min_gq=None, shifts=(0, 7)):
    """the host form and the device form, text and BCF, against the restatement"""
    g1, g2, gq, cov, vao, probs, vgo, status = case
    want_t, off_t = expect_text(g1, g2, gq, haploid, vao, probs, vgo, status, cov, min_gq)
    want_b, off_b = expect_bcf(g1, g2, gq, haploid, keys, vao, probs, vgo, status, cov, min_gq)
    got, off = ctx.format_calls_gp(g1, g2, gq, haploid, vao, probs, vgo, status, cov=cov, min_gq=min_gq)
    assert np.array_equal(off, off_t) and len(got) == len(want_t)
    assert got == want_t
    assert all(np.isfinite(m) and m >= 0 for m in ctx.format_stats())
    got, off = ctx.encode_calls_bcf_gp(g1, g2, gq, haploid, keys, vao, probs, vgo, status, cov=cov, min_gq=min_gq)
    assert np.array_equal(off, off_b) and len(got) == len(want_b)
    assert got == want_b
    assert all(np.isfinite(m) and m >= 0 for m in ctx.bcf_stats())
    for shift in shifts:
        for bcf, want, want_off in ((False, want_t, off_t), (True, want_b, off_b)):
            rc, need, out, guard, doff = _device_form(ctx, bcf, case, haploid, keys, min_gq, len(want), shift=shift)
            assert rc == 0 and need == len(want) and np.array_equal(doff, want_off)
            assert out == want and (guard == 0xAA).all()
    return want_t, want_b


# ---- the values -----------------------------------------------------------------------------------------------------------------

def test_the_restatement_knows_the_edges():
    assert ["%.6f" % x for x in (1 / 128, 3 / 128, 127 / 128)] == ["0.007812", "0.023438", "0.992188"]           # the exact ties, to even
    assert ["%.6f" % x for x in (4.9999999e-7, 5e-7, 5.0000001e-7)] == ["0.000000", "0.000000", "0.000001"]       # (5e-7 the double lies below 5e-7)
    assert "%.6f" % math.nextafter(1.0, 0.0) == "1.000000" and "%.6f" % 5e-324 == "0.000000"
    assert all(printable(x) for x in PRINTABLE) and not any(printable(x) for x in UNPRINTABLE)
    assert int(np.float32(1e-40).view(np.uint32)) == 0x000116C2                    # a float denormal, kept
    assert vcf_order(3, False) == [0, 1, 3, 2, 4, 5]                               # 0/0 0/1 1/1 0/2 1/2 2/2 out of 0/0 0/1 0/2 1/1 1/2 2/2


@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
def test_every_edge_value(ctx, haploid):
    """each edge value in the first, a middle and the last place of a list, in the first and the last plane; a record of each status
    that has no list, its probs garbage"""
    vals = PRINTABLE + UNPRINTABLE
    A = 3
    G = n_gt(A, haploid)
    n = len(vals) + 3
    P = 2
    case = list(_case(P, [A] * n, haploid, seed=3, values=[0.25]))
    g1, g2, gq, cov, vao, probs, vgo, status = case
    status[:] = 0
    probs[:] = 0.25
    for v, x in enumerate(vals):
        probs[0, int(vgo[v])] = x
        probs[0, int(vgo[v]) + G // 2] = x
        probs[1, int(vgo[v + 1]) - 1] = x
    for s in (1, 2, 3):
        v = len(vals) + s - 1
        status[:, v] = s
        probs[:, int(vgo[v]):int(vgo[v + 1])] = np.resize(np.array(GARBAGE), G)
    text, bcf = _both(ctx, case, haploid)
    rows = text.decode().split("\n")
    assert rows[PRINTABLE.index(1 / 128)].split("\t")[1].split(":")[3].split(",")[0] == "0.007812"
    assert rows[PRINTABLE.index(127 / 128)].split("\t")[2].split(":")[3].split(",")[-1] == "0.992188"
    assert rows[len(PRINTABLE)].split("\t")[1].split(":")[3].split(",")[0] == "."                        # NaN
    assert all(c.split(":")[3] == "." for r in rows[len(vals):len(vals) + 3] for c in r.split("\t")[1:])    # no list: one '.'
    assert struct.pack("<I", 0x000116C2) in bcf and struct.pack("<II", F_MISSING, F_EOV) in bcf


# ---- the shapes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_cov", [False, True], ids=["gt-gq-gp", "gt-gq-covs-gp"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 2, 63, 64])
def test_gp_is_exact(ctx, planes, haploid, with_cov):
    """33 records (two write tiles) of 1, 2, 3, 5 alleles (diploid A = 5: G = 15, the long desc) and, haploid, 14, 15, 16; with and
    without the mask"""
    alleles = ([1, 2, 3, 5, 14, 15, 16] if haploid else [1, 2, 3, 5, 2, 3, 4]) * 5
    case = _case(planes, alleles[:33], haploid, seed=planes * 10 + 2 * haploid + with_cov, with_cov=with_cov)
    keys = (1, 127, 128, 32768) if planes == 2 else (1, 2, 3, 4)
    for min_gq in (None, 50):
        text, _ = _both(ctx, case, haploid, keys, min_gq, shifts=(1, 15) if min_gq else (0, 7))
        if min_gq:
            assert (b"\t.:" in text) if haploid else (b"\t./.:" in text)


def test_no_record(ctx):
    z = np.zeros((2, 0), dtype=np.int32)
    one32, one64 = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    probs, status = np.zeros((2, 0)), np.zeros((2, 0), dtype=np.uint8)
    assert ctx.format_calls_gp(z, z, z, False, one32, probs, one64, status)[0] == b""
    out, off = ctx.encode_calls_bcf_gp(z, z, z, False, (1, 2, 3, 4), one32, probs, one64, status)
    assert out == b"" and list(off) == [0]
    for bcf in (False, True):
        rc, need, out, guard, doff = _device_form(ctx, bcf, (z, z, z, None, one32, probs, one64, status), False, (1, 2, 3, 4), None, 0)
        assert rc == 0 and need == 0 and list(doff) == [0] and (guard == 0xAA).all()


def test_rows_across_the_window_boundary(ctx):
    """rows of about 1.1 KB (text) at 64 planes: 33 of them pass the 16 KB window of a write tile twice, a row -- and a value --
    on each boundary"""
    case = _case(64, [2] * 33, True, seed=9, with_cov=False)
    text, bcf = _both(ctx, case, True, shifts=(0, 15))
    assert len(text) > 2 * 16384


def test_one_record_of_many_windows(ctx):
    """130 alleles, diploid, 64 planes: G = 8515, one row of about 4.9 MB through about 300 windows of the text's write pass"""
    case = _case(64, [130], False, seed=10, with_cov=False)
    text, bcf = _both(ctx, case, False, shifts=(7,))
    assert len(text) > 4_000_000 and len(bcf) == 2 + 1 + 128 + 2 + 1 + 64 + 2 + 4 + 64 * 8515 * 4


@pytest.mark.parametrize("bcf", [False, True], ids=["text", "bcf"])
def test_buffer_too_small(ctx, bcf):
    """the capacity one byte short, and cutting inside a GP value: MG_ERR_LIMIT, the size right, row_off whole, the guard at and behind
    the capacity untouched -- host form and device form"""
    haploid, keys = False, (1, 2, 3, 4)
    case = _case(3, [2, 3, 1, 5] * 9, haploid, seed=12)
    g1, g2, gq, cov, vao, probs, vgo, status = case
    status[:, 20] = 0
    probs[:, int(vgo[20]):int(vgo[21])] = 0.5
    want, want_off = (expect_bcf(g1, g2, gq, haploid, keys, vao, probs, vgo, status, cov) if bcf else expect_text(g1, g2, gq, haploid, vao, probs, vgo, status, cov))
    n, P = len(vao) - 1, 3
    if bcf:
        inside = int(want_off[21]) - 4 * 3 * n_gt(int(vao[21]) - int(vao[20]), haploid) + 6   # two bytes into the second float of record 20's first plane
        assert want[inside - 2:inside + 2] == struct.pack("<f", 0.5)
    else:
        inside = int(want_off[21]) - 5                                              # "0.500000\n": four digits of the last value are cut
        assert want[inside - 4:inside + 5] == b"0.500000\n"
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for cap in (inside, len(want) - 1):
        buf = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
        off = np.full(n + 1, 1 << 63, dtype=np.uint64)
        need = C.c_uint64(0)
        if bcf:
            call = lambda c: ctx._L.mg_encode_calls_bcf(ctx.h, C.byref(Cells(n, P, int(haploid), p(g1), p(g2), p(gq), 0, 0, p(cov), p(vao), p(probs), p(vgo), p(status), None, None,
                                                                          CELLS_GP)), C.byref(BcfKeys(*keys)), p(buf) if c else None, c, p(off), C.byref(need))
        else:
            call = lambda c: ctx._L.mg_format_calls(ctx.h, C.byref(Cells(n, P, int(haploid), p(g1), p(g2), p(gq), 0, 0, p(cov), p(vao), p(probs), p(vgo), p(status), None, None,
                                                                      CELLS_GP)), p(buf) if c else None, c, p(off), C.byref(need))
        assert call(cap) == MG_ERR_LIMIT and need.value == len(want)
        assert np.array_equal(off, want_off)
        assert (buf[cap:] == 0xAA).all()
        assert buf[:cap].tobytes() == want[:cap]
        assert call(need.value) == 0 and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
        for shift in (0, 7):
            rc, dneed, out, guard, doff = _device_form(ctx, bcf, case, haploid, keys, None, cap, guard=4096, shift=shift)
            assert rc == MG_ERR_LIMIT and dneed == len(want)
            assert np.array_equal(doff, want_off)
            assert out == want[:cap]
            assert (guard == 0xAA).all(), "bytes at or behind the capacity were written"
    with pytest.raises(MalvaError) as e:
        (ctx.encode_calls_bcf_gp(g1, g2, gq, haploid, keys, vao, probs, vgo, status, cov=cov, out_cap=len(want) - 1) if bcf else
         ctx.format_calls_gp(g1, g2, gq, haploid, vao, probs, vgo, status, cov=cov, text_cap=len(want) - 1))
    assert e.value.code == MG_ERR_LIMIT and e.value.needed == len(want) and np.array_equal(e.value.row_off, want_off)


def test_arguments(ctx):
    g = np.zeros((2, 2), dtype=np.int32)
    vao, vgo = np.array([0, 2, 4], dtype=np.uint32), np.array([0, 3, 6], dtype=np.uint64)
    probs, status = np.zeros((2, 6)), np.zeros((2, 2), dtype=np.uint8)
    with pytest.raises(MalvaError, match="required"):
        ctx.format_calls_gp(g, g, g, False, None, probs, vgo, status)
    with pytest.raises(MalvaError, match="required"):
        ctx.encode_calls_bcf_gp(g, g, g, False, (1, 2, 3, 4), vao, probs, None, status)
    with pytest.raises(MalvaError, match="NULL"):
        ctx.format_calls_gp(g, g, g, False, vao, None, vgo, status)
    with pytest.raises(MalvaError, match="dictionary"):
        ctx.encode_calls_bcf_gp(g, g, g, False, (1, 2, 3, -4), vao, probs, vgo, status)
    with pytest.raises(MalvaError, match="n_planes"):
        ctx.format_calls_gp(np.zeros((65, 2), dtype=np.int32), g, g, False, vao, probs, vgo, status)


# ---- the command line ---------------------------------------------------------------------------------------------------------

def _cli(args, env=None, binary=False):
    r = subprocess.run([BIN] + args, capture_output=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout if binary else r.stdout.decode()


K, REF_K, N_SAMPLES = 35, 43, 4


@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    """diploid: the synthetic panel of indel / MNP clusters (multi-allelic records) and four samples, as tests/test_gpu_bcf.py builds
    it; haploid: tests/golden/haploid.* with three samples (the golden reads, and two sets simulated from the panel)"""
    from test_gpu_bcf import _sample_table
    from test_gpu_reads import simulate_reads
    import gzip
    out = {}
    d = tmp_path_factory.mktemp("gp_diploid")
    panel = synth.indel_panel(600, seed=21, n_samples=70)
    base = synth.flat_kmer_table(panel, 30_000, K, REF_K, seed=5, max_records=500)
    prefix = str(d / "p")
    synth.write_vcf_fasta(panel, prefix)
    names = ["s%d" % s for s in range(N_SAMPLES)]
    for s in range(N_SAMPLES):
        hi, lo, cnt = _sample_table(base, s, False)
        rows = synth.unpack_ascii(hi, lo, REF_K)
        with open(str(d / ("s%d.txt" % s)), "w") as fh:
            for r, c in zip(rows, cnt):
                fh.write("%s\t%d\n" % (bytes(r[:REF_K]).decode(), int(c)))
    (d / "cohort.tsv").write_text("".join("%s\t%s\n" % (n, n) for n in names))
    common = ["-k", str(K), "-r", str(REF_K), "-b", "1", prefix + ".fa", prefix + ".vcf"]
    env = dict(os.environ, MALVA_GENO_BF_BITS=str(1 << 26), MALVA_GENO_BATCH="150")
    _cli(["index"] + common + [str(d / "s0")], env=env)
    out["diploid"] = (d, common, env, names)

    d = tmp_path_factory.mktemp("gp_haploid")
    fa = os.path.join(GOLDEN, "haploid.fa")
    vcf = str(d / "haploid.vcf.gz")
    shutil.copy(os.path.join(GOLDEN, "haploid.vcf.gz"), vcf)
    shutil.copy(os.path.join(GOLDEN, "haploid.fq"), str(d / "haploid.fq"))
    contigs, name = {}, None
    for line in open(fa):
        if line.startswith(">"):
            name = line[1:].split()[0]
            contigs[name] = []
        else:
            contigs[name].append(line.strip().upper())
    contigs = {n: "".join(v) for n, v in contigs.items()}
    records = []
    for line in gzip.open(vcf, "rt"):
        if not line.startswith("#"):
            f = line.split("\t")
            records.append((f[0], int(f[1]) - 1, f[3], f[4].split(",")))
    simulate_reads(contigs, records, 71, str(d / "sim1.fq"), True)
    simulate_reads(contigs, records, 72, str(d / "sim2.fq"), True)
    names = ["reads", "sim1", "sim2"]
    (d / "cohort.tsv").write_text("reads\thaploid.fq\nsim1\tsim1.fq\nsim2\tsim2.fq\n")
    common = ["-1", "-k", str(K), "-r", str(REF_K), "-b", "1", "-f", "AF", fa, vcf]
    env = dict(os.environ, MALVA_GENO_BATCH="37")
    _cli(["index"] + common + [str(d / "haploid.fq")], env=env)
    out["haploid"] = (d, common, env, names)
    return out


def _run(cohorts, mode, opts, target, fmt=None, env=None):
    d, common, env0, names = cohorts[mode]
    return _cli(["call", "--cohort"] + list(opts) + ["--merged", target] + ([] if fmt is None else ["--merged-format", fmt]) + common + [str(d / "cohort.tsv")],
                env=dict(env0, **(env or {})), binary=True)


def _records(text):
    return [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]


def _gts(info):
    """INFO of a per-sample -v record -> the list behind GTS= as (genotype, number) pairs"""
    gts = dict(kv.split("=", 1) for kv in info.split(";"))["GTS"]
    return [tuple(e.split(":")) for e in gts.split(",")]


@pytest.mark.parametrize("mode", ["haploid", "diploid"])
def test_cli_gp_is_the_per_sample_gts(cohorts, tmp_path, mode):
    """-v -o DIR --merged M --gp: a cell's GP, put back into the reference's order, is string for string the numbers behind GTS= of the
    sample's own file where that list is a normal one and '.' where it is an early-out list; the rest of the line is the merged
    file made without --gp"""
    d, common, env0, names = cohorts[mode]
    haploid = mode == "haploid"
    with_gp, without = str(tmp_path / "gp.vcf"), str(tmp_path / "plain.vcf")
    assert _run(cohorts, mode, ["-v", "-o", str(tmp_path / "o"), "--gp"], with_gp) == b""
    assert _run(cohorts, mode, ["-v"], without) == b""
    head = [l for l in open(with_gp).read().split("\n") if l.startswith("##")]
    head0 = [l for l in open(without).read().split("\n") if l.startswith("##")]
    at = [i for i, l in enumerate(head) if l.startswith("##FORMAT=<ID=GP,Number=G,Type=Float,")]
    assert len(at) == 1 and head[at[0] - 1].startswith("##FORMAT=<ID=COVS,") and head[:at[0]] + head[at[0] + 1:] == head0
    got, plain = _records(open(with_gp).read()), _records(open(without).read())
    singles = [_records(open(str(tmp_path / "o" / (n + ".vcf"))).read()) for n in names]
    assert len(got) == len(plain) == len(singles[0]) and len(got) > 100
    normal = early = multi = 0
    for i, (g, w) in enumerate(zip(got, plain)):
        assert g[:8] == w[:8] and g[8] == "GT:GQ:COVS:GP" and w[8] == "GT:GQ:COVS"
        A = 1 + (0 if g[4] == "." else 1 + g[4].count(","))
        for s in range(len(names)):
            cell, gp = g[9 + s].rsplit(":", 1)
            assert cell == w[9 + s], "record %d sample %d" % (i, s)
            lst = _gts(singles[s][i][7])
            names_want = ["%d" % a if haploid else "%d/%d" % (a, c) for a in range(A) for c in range(a, a + 1 if haploid else A)]
            if [x[0] for x in lst] == names_want and A > 1:                         # a normal list: every genotype once, in the reference's order
                vals = gp.split(",")
                assert len(vals) == len(lst), "record %d sample %d" % (i, s)
                back = [vals[c * (c + 1) // 2 + a] for a in range(A) for c in range(a, A)] if not haploid else vals
                assert back == [x[1] if x[1] != "-nan" else "." for x in lst], "record %d sample %d" % (i, s)
                normal += 1
                multi += A > 2
            else:
                assert gp == ".", "record %d sample %d: %s against %s" % (i, s, gp, lst)
                early += 1
    assert normal > 100 and early > 0 and (haploid or multi > 0)
    assert sorted(os.listdir(tmp_path)) == ["gp.vcf", "o", "plain.vcf"]


def test_cli_gp_without_verbose_and_the_out_dir(cohorts, tmp_path):
    """without -v FORMAT is GT:GQ:GP and the GP are those of the -v run; the files of -o are byte for byte those of a run without --gp"""
    d, common, env0, names = cohorts["diploid"]
    _run(cohorts, "diploid", ["-o", str(tmp_path / "a"), "--gp"], str(tmp_path / "a.vcf"))
    _run(cohorts, "diploid", ["-o", str(tmp_path / "b")], str(tmp_path / "b.vcf"))
    _run(cohorts, "diploid", ["-v", "--gp"], str(tmp_path / "v.vcf"))
    for n in names:
        assert open(str(tmp_path / "a" / (n + ".vcf")), "rb").read() == open(str(tmp_path / "b" / (n + ".vcf")), "rb").read(), n
    a, b, v = (_records(open(str(tmp_path / f)).read()) for f in ("a.vcf", "b.vcf", "v.vcf"))
    assert len(a) == len(b) == len(v) > 100
    for ra, rb, rv in zip(a, b, v):
        assert ra[:8] == rb[:8] and ra[8] == "GT:GQ:GP" and rb[8] == "GT:GQ"
        assert [c.rsplit(":", 1)[0] for c in ra[9:]] == rb[9:]
        assert [c.rsplit(":", 1)[1] for c in ra[9:]] == [c.rsplit(":", 1)[1] for c in rv[9:]]
    text = open(str(tmp_path / "a.vcf")).read()
    assert text.count("##FORMAT=<ID=GP,") == 1 and "##FORMAT=<ID=COVS" not in text


def test_cli_gp_keeps_its_values_under_the_mask(cohorts, tmp_path):
    from test_gpu_bcf import _median_gq
    _run(cohorts, "diploid", ["--gp"], str(tmp_path / "a.vcf"))
    a = open(str(tmp_path / "a.vcf")).read()
    q = _median_gq(a)
    _run(cohorts, "diploid", ["--gp", "--min-gq", str(q), "--site-tags"], str(tmp_path / "m.vcf"))
    masked = 0
    for ra, rm in zip(_records(a), _records(open(str(tmp_path / "m.vcf")).read())):
        for ca, cm in zip(ra[9:], rm[9:]):
            gt, gq, gp = ca.split(":")
            if int(gq) < q:
                assert cm == "./.:%s:%s" % (gq, gp)
                masked += 1
            else:
                assert cm == ca
    assert masked > 0


def _gp_bits(key, bits):
    """how the decoder of tests/test_bcf_out_cpu.py prints a float: GP as its bits, to be held against the text; the others as
    tests/test_gpu_bcf.py reads them"""
    from test_gpu_bcf import _af_text
    return "%08x" % bits if key == "GP" and bits != F_MISSING else _af_text(key, bits)


@pytest.mark.parametrize("mode", ["haploid", "diploid"])
def test_cli_gp_in_bcf_and_whatever_the_grouping(cohorts, tmp_path, mode):
    """vcf, ubcf and bcf with --cohort-group 1 and with the default are one file each (bcf: its members inflated), the ubcf in groups
    of two and other batches too (haploid: vcf and ubcf alone); the BCF decodes to the text in everything but GP, in GP it agrees in missingness exactly and in value within
    5e-7 + 2^-25: the text is within half a millionth of the double, the float within half an ulp of a value <= 1 of it"""
    opts = ["-v", "--gp", "--site-tags"]
    files = {}
    fmts = ("vcf", "ubcf", "bcf") if mode == "diploid" else ("vcf", "ubcf")
    made = []
    for fmt in fmts:
        for tag, group, batch in (("all", [], None), ("g1", ["--cohort-group", "1"], None), ("g2", ["--cohort-group", "2"], "11")):
            if tag == "g2" and (fmt != "ubcf" or mode != "diploid"):
                continue
            made.append("%s.%s" % (tag, fmt))
            target = str(tmp_path / ("%s.%s" % (tag, fmt)))
            assert _run(cohorts, mode, opts + group, target, fmt, env={"MALVA_GENO_BATCH": batch} if batch else None) == b""
            data = open(target, "rb").read()
            files[fmt, tag] = b"".join(raw for _, raw in bgzf_members(data)) if fmt == "bcf" else data
        assert files[fmt, "all"] == files[fmt, "g1"] == files.get((fmt, "g2"), files[fmt, "all"]), "the %s file depends on the grouping or the batching" % fmt
    assert files.get(("bcf", "all"), files["ubcf", "all"]) == files["ubcf", "all"]
    assert sorted(os.listdir(tmp_path)) == sorted(made)
    text = _records(files["vcf", "all"].decode())
    lines = bcf_to_vcf(files["ubcf", "all"], float_text=_gp_bits)
    assert [l for l in lines if l.startswith("##FORMAT=<ID=GP,")]
    binary = _records("\n".join(lines))
    assert len(text) == len(binary) > 100
    bound = 5e-7 + 2.0 ** -25
    values = missing = 0
    for rt, rb in zip(text, binary):
        assert rt[:8] == rb[:8] and rt[8] == rb[8] == "GT:GQ:COVS:GP"
        for ct, cb in zip(rt[9:], rb[9:]):
            assert ct.rsplit(":", 1)[0] == cb.rsplit(":", 1)[0]
            gt, gb = ct.rsplit(":", 1)[1].split(","), cb.rsplit(":", 1)[1].split(",")
            assert len(gt) == len(gb) and [x == "." for x in gt] == [x == "." for x in gb]
            for x, y in zip(gt, gb):
                if x == ".":
                    missing += 1
                    continue
                f = struct.unpack("<f", struct.pack("<I", int(y, 16)))[0]
                assert abs(float(x) - f) <= bound, (x, y)
                values += 1
    assert values > 1000 and missing > 0
