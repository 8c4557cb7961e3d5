"""`call --cohort --merged`: one multi-sample VCF whose sample columns are made on the device (mg_format_calls).

The ABI is compared byte for byte with a formatter written here (str() of Python ints is std::to_string(int)); the command
line with the column paste of the single `call` outputs it replaces.  Every comparison is exact."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from malva_amd import Context, MalvaError, synth
from malva_amd.capi import Cells

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
MG_ERR_LIMIT, MG_ERR_STATE = -5, -3
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
EDGES = np.array([0, 9, 10, 99, 100, 127, 128, INT_MAX, -1, INT_MIN, 1, 999, 1000, 99999, 100000, 999999999, 1000000000, -9, -10, -2147483647], dtype=np.int64)
COV_EDGES = np.array([0, 1, 9, 10, 200, 201, 65535, INT_MAX, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 3000000000], dtype=np.int64)


# ---- the formatters of the test ---------------------------------------------------------------------------------------------

def format_plain(g1, g2, gq, haploid, cov=None, vao=None):
    """-> (bytes, row_off), one str() per number"""
    P, n = g1.shape
    rows = []
    for v in range(n):
        cells = []
        for p in range(P):
            c = str(int(g1[p, v])) if haploid else "%d/%d" % (int(g1[p, v]), int(g2[p, v]))
            c += ":%d" % int(gq[p, v])
            if cov is not None:
                c += ":" + ",".join(str(int(np.int32(np.uint32(x)))) for x in cov[p, vao[v]:vao[v + 1]])
            cells.append("\t" + c)
        rows.append("".join(cells) + "\n")
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return "".join(rows).encode(), off


def _int_len(x):
    m = np.abs(x)
    nd = np.ones(x.shape, dtype=np.int64)
    for d in range(1, 10):
        nd += m >= 10 ** d
    return nd + (x < 0)


def _put_int(out, pos, x):
    """decimal text of the int64 values x at byte positions pos"""
    ln = _int_len(x)
    neg = x < 0
    out[pos[neg]] = ord("-")
    m = np.abs(x)
    last = pos + ln - 1
    nd = ln - neg
    for d in range(10):
        sel = nd > d
        out[last[sel] - d] = ord("0") + (m[sel] // 10 ** d) % 10


def format_numpy(g1, g2, gq, haploid, cov=None, vao=None):
    """the same text laid out with array arithmetic (for the sizes format_plain would take minutes for); the two are held against
    each other on every small case"""
    P, n = g1.shape
    a1, a2, q = (x.astype(np.int64).T for x in (g1, g2, gq))                    # [n, P]
    l1, l2, lq = _int_len(a1), _int_len(a2), _int_len(q)
    fixed = 1 + l1 + (0 if haploid else 1 + l2) + 1 + lq
    if cov is not None:
        cv = cov.astype(np.uint32).view(np.int32).astype(np.int64)                # [P, slots], the (int) cast
        cl = 1 + _int_len(cv)
        ccum = np.zeros((P, cv.shape[1] + 1), dtype=np.int64)
        ccum[:, 1:] = np.cumsum(cl, axis=1)
        lo, hi = vao[:-1].astype(np.int64), vao[1:].astype(np.int64)
        cov_len = (ccum[:, hi] - ccum[:, lo]).T                                   # [n, P]
        assert (hi > lo).all()
    else:
        cov_len = 0
    cell = fixed + cov_len
    row_len = cell.sum(axis=1) + 1
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(row_len)
    start = off[:-1, None] + np.cumsum(cell, axis=1) - cell
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    out[start] = ord("\t")
    at = start + 1
    _put_int(out, at.ravel(), a1.ravel())
    at = at + l1
    if not haploid:
        out[at] = ord("/")
        _put_int(out, (at + 1).ravel(), a2.ravel())
        at = at + 1 + l2
    out[at] = ord(":")
    _put_int(out, (at + 1).ravel(), q.ravel())
    if cov is not None:
        A = (hi - lo)
        rec = np.repeat(np.arange(n), A)                                          # record of every slot
        first = np.zeros(cv.shape[1], dtype=bool)
        first[lo] = True
        for p in range(P):
            pos = (start[:, p] + fixed[:, p])[rec] + ccum[p, :-1] - ccum[p, lo][rec]
            out[pos] = np.where(first, ord(":"), ord(","))
            _put_int(out, pos + 1, cv[p])
    out[off[1:] - 1] = ord("\n")
    return out.tobytes(), off.astype(np.uint64)


def _case(planes, n, haploid, with_cov, seed):
    rng = np.random.default_rng(seed)

    def draw(shape, edges, lo, hi):
        """the edge values, numbers as a call gives them (0 .. 299), and anything else of the range; mostly the second at the large size,
        which keeps its text near 0.1 GB"""
        x = rng.integers(lo, hi, size=shape, dtype=np.int64)
        pick = rng.random(shape) < (0.5 if n <= 300 else 0.05)
        x[pick] = edges[rng.integers(0, len(edges), size=int(pick.sum()))]
        small = ~pick & (rng.random(shape) < (0.5 if n <= 300 else 0.95))
        x[small] = rng.integers(0, 300, size=int(small.sum()))
        return x
    g1, g2, gq = (draw((planes, n), EDGES, INT_MIN, INT_MAX + 1).astype(np.int32) for _ in range(3))
    if n:                                                                          # every edge value in gq, in the first and last plane
        for j, e in enumerate(EDGES):
            gq[0, j % n] = e
            gq[planes - 1, (n - 1 - j) % n] = e
    if haploid:
        g2[:] = -1
    cov = vao = None
    if with_cov:
        A = 1 + np.arange(n) % 130 if n <= 300 else np.where(np.arange(n) % 10007 < 130, 1 + np.arange(n) % 10007 % 130, 1 + np.arange(n) % 3)
        vao = np.zeros(n + 1, dtype=np.uint32)
        vao[1:] = np.cumsum(A)
        cov = draw((planes, int(vao[-1])), COV_EDGES, 0, 1 << 32).astype(np.uint32)
    return g1, g2, gq, cov, vao


# ---- the ABI ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def _device_form(ctx, g1, g2, gq, haploid, cov, vao, cap, guard=64, shift=0):
    """-> (rc, need, text bytes [cap], guard bytes, row_off); the text buffer starts `shift` bytes into its allocation"""
    dev = torch.device("cuda", 0)
    P, n = g1.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)).view(np.int32)).to(dev)
    d1, d2, dq, dc, dv = t(g1), t(g2), t(gq), t(cov), t(vao)
    text = torch.full((shift + cap + guard,), 0xAA, dtype=torch.uint8, device=dev)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ptr = lambda x: 0 if x is None else x.data_ptr()
    rc, need = ctx.format_calls_device(n, P, haploid, ptr(d1), ptr(d2), ptr(dq), ptr(dc), ptr(dv), text.data_ptr() + shift if cap else 0, cap, off.data_ptr())
    ctx.synchronize()
    h = text.cpu().numpy()
    assert (h[:shift] == 0xAA).all(), "bytes in front of the buffer were written"
    return rc, need, h[shift:shift + cap].tobytes(), h[shift + cap:], off.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n", [0, 1, 257, 100003])
@pytest.mark.parametrize("with_cov", [False, True], ids=["gt-gq", "gt-gq-covs"])
@pytest.mark.parametrize("haploid", [True, False], ids=["haploid", "diploid"])
@pytest.mark.parametrize("planes", [1, 3, 16, 17, 64])
def test_format_calls_is_exact(ctx, planes, haploid, with_cov, n):
    g1, g2, gq, cov, vao = _case(planes, n, haploid, with_cov, seed=planes * 1000 + n % 997 + 2 * haploid + with_cov)
    want, want_off = format_numpy(g1, g2, gq, haploid, cov, vao)
    if n <= 257:
        plain, plain_off = format_plain(g1, g2, gq, haploid, cov, vao)
        assert plain == want and np.array_equal(plain_off, want_off), "the two formatters of the test disagree"
        if n >= 257:
            for e in EDGES:
                assert (":%d" % e).encode() in want
    got, off = ctx.format_calls(g1, g2, gq, haploid, cov, vao)
    assert np.array_equal(off, want_off)
    assert len(got) == len(want)
    assert got == want
    ms = ctx.format_stats()
    assert len(ms) == 3 and all(m >= 0 for m in ms)
    for shift in (0, 5):                                                          # the device form; once into a buffer that is not 16-byte aligned
        rc, need, text, guard, doff = _device_form(ctx, g1, g2, gq, haploid, cov, vao, len(want), shift=shift)
        assert rc == 0 and need == len(want)
        assert np.array_equal(doff, want_off)
        assert text == want
        assert (guard == 0xAA).all()


@pytest.mark.parametrize("with_cov", [False, True], ids=["gt-gq", "gt-gq-covs"])
@pytest.mark.parametrize("planes,n", [(1, 1), (3, 257), (17, 5000), (64, 40000)])
def test_buffer_too_small(ctx, planes, n, with_cov):
    """text_cap one byte short, and 0: MG_ERR_LIMIT with the exact size, row_off valid, nothing at or behind text_cap touched, the bytes
    in front of it the text's first, and the call with the size it reported succeeds -- host form and device form"""
    haploid = planes == 3
    g1, g2, gq, cov, vao = _case(planes, n, haploid, with_cov, seed=77 + planes)
    want, want_off = format_numpy(g1, g2, gq, haploid, cov, vao)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for cap in (len(want) - 1, 0):
        buf = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
        off = np.full(n + 1, 1 << 63, dtype=np.uint64)
        need = C.c_uint64(0)
        rc = ctx._L.mg_format_calls(ctx.h, C.byref(Cells(n, planes, int(haploid), p(g1), p(g2), p(gq), 0, 0, p(cov), p(vao))), p(buf) if cap else None, cap, p(off), C.byref(need))
        assert rc == MG_ERR_LIMIT and need.value == len(want)
        assert np.array_equal(off, want_off)
        assert (buf[cap:] == 0xAA).all()
        assert buf[:cap].tobytes() == want[:cap]
        rc = ctx._L.mg_format_calls(ctx.h, C.byref(Cells(n, planes, int(haploid), p(g1), p(g2), p(gq), 0, 0, p(cov), p(vao))), p(buf), need.value, p(off), C.byref(need))
        assert rc == 0 and need.value == len(want) and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
        for shift in (0, 7):
            rc, dneed, text, guard, doff = _device_form(ctx, g1, g2, gq, haploid, cov, vao, cap, guard=4096, shift=shift)
            assert rc == MG_ERR_LIMIT and dneed == len(want)
            assert np.array_equal(doff, want_off)
            assert text == want[:cap]
            assert (guard == 0xAA).all(), "bytes behind text_cap were written"
            rc, dneed, text, guard, doff = _device_form(ctx, g1, g2, gq, haploid, cov, vao, dneed, shift=shift)
            assert rc == 0 and text == want and (guard == 0xAA).all()
    with pytest.raises(MalvaError) as e:                                          # the binding hands the size and the offsets on
        ctx.format_calls(g1, g2, gq, haploid, cov, vao, text_cap=len(want) - 1)
    assert e.value.code == MG_ERR_LIMIT and e.value.needed == len(want) and np.array_equal(e.value.row_off, want_off)


def test_format_stats_before_the_first_call_and_after_an_empty_one():
    with Context(35, 43, 1 << 20) as c:
        with pytest.raises(MalvaError) as e:
            c.format_stats()
        assert e.value.code == MG_ERR_STATE
        g = np.zeros((2, 0), dtype=np.int32)
        text, off = c.format_calls(g, g, g, False)                                # no record: the call still counts as one
        assert text == b"" and list(off) == [0]
        ms = c.format_stats()
        assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)


def test_format_calls_arguments(ctx):
    g = np.zeros((65, 2), dtype=np.int32)
    with pytest.raises(MalvaError, match="n_planes"):
        ctx.format_calls(g, g, g, False)
    g = np.zeros((2, 2), dtype=np.int32)
    with pytest.raises(MalvaError, match="go together"):
        ctx.format_calls(g, g, g, False, cov=np.zeros((2, 2), dtype=np.uint32))
    text, off = ctx.format_calls(g, None, g, True)                               # haploid: gt2 is not read
    assert text == b"\t0:0\t0:0\n" * 2 and list(off) == [0, 9, 18]


# ---- the command line ---------------------------------------------------------------------------------------------------------

def _cli(args, env=None):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _split(text):
    lines = text.split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    head = [l for l in lines if l.startswith("#")]
    return head, lines[len(head):]


def check_paste(merged, singles, names, plain_header=None):
    """merged: the multi-sample text; singles: the single `call` outputs in manifest order.  plain_header given: the singles are
    verbose outputs (COVS / GTS in INFO) and plain_header the header of a plain single call."""
    verbose = plain_header is not None
    head, recs = _split(merged)
    s_head, s_recs = zip(*(_split(t) for t in singles))
    want_head = list(plain_header if verbose else s_head[0])
    assert want_head[-1].split("\t")[:9] == "#CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split() and len(want_head[-1].split("\t")) == 10
    want_head[-1] = "\t".join(want_head[-1].split("\t")[:9] + list(names))
    if verbose:
        want_head.insert(len(want_head) - 1, '##FORMAT=<ID=COVS,Number=R,Type=Integer,Description="Allele coverages">')
        assert not any(l.startswith("##INFO=<ID=COVS") or l.startswith("##INFO=<ID=GTS") for l in head)
    assert head == want_head
    assert len(recs) == len(s_recs[0]) > 0 and all(len(r) == len(recs) for r in s_recs)
    for i, line in enumerate(recs):
        cols = [r[i].split("\t") for r in s_recs]
        assert all(len(c) == 10 and c[:7] == cols[0][:7] for c in cols)
        if not verbose:
            want = cols[0][:9] + [c[9] for c in cols]
        else:
            cells = []
            for c in cols:
                assert c[8] == "GT:GQ"
                info = dict(kv.split("=", 1) for kv in c[7].split(";"))
                cells.append(c[9] + ":" + info["COVS"])
            want = cols[0][:7] + [".", "GT:GQ:COVS"] + cells
        assert line == "\t".join(want), "record %d" % i
    return recs


@pytest.fixture(scope="module")
def haploid_cohort(tmp_path_factory, golden_dir):
    """the four-sample manifest of tests/test_gpu_cohort.py::test_cli_cohort_of_four_equals_four_single_calls"""
    from oracle import kmc_standin
    from test_gpu_reads import simulate_reads, write_dump
    tmp = tmp_path_factory.mktemp("merged")
    fa = os.path.join(golden_dir, "haploid.fa")
    vcf = str(tmp / "haploid.vcf.gz")
    shutil.copy(os.path.join(golden_dir, "haploid.vcf.gz"), vcf)
    fq = str(tmp / "haploid.fq")
    shutil.copy(os.path.join(golden_dir, "haploid.fq"), fq)
    write_dump(str(tmp / "dump.txt"), kmc_standin.count_fastq(fq, 43))
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
    simulate_reads(contigs, records, 71, str(tmp / "sim1.fq"), True)
    simulate_reads(contigs, records, 72, str(tmp / "sim2.fq"), True)
    hdr = [l for l in gzip.open(vcf, "rt") if l.startswith("#CHROM")][0].rstrip("\n").split("\t")[9:]
    (tmp / "keep.txt").write_text("\n".join(hdr[:max(1, len(hdr) // 2)]) + "\n")
    inputs = {"reads": "haploid.fq", "dump": "dump", "sim1": "sim1.fq", "sim2": "sim2.fq,sim1.fq"}
    (tmp / "cohort.tsv").write_text("# name<tab>input\n\n" + "".join("%s\t%s\n" % kv for kv in inputs.items()))
    return tmp, fa, vcf, fq, inputs


COMMON = ["-1", "-k", "35", "-r", "43", "-b", "1", "-f", "AF"]


def _singles(tmp, fa, vcf, inputs, opts):
    return [_cli(["call"] + COMMON + opts + [fa, vcf, ",".join(str(tmp / x) for x in inp.split(","))]) for inp in inputs.values()]


def _no_leftovers(directory, allowed):
    left = sorted(set(os.listdir(directory)) - set(allowed))
    assert not left, "left beside the output: %s" % left


def test_cli_merged_is_the_paste_of_four_single_calls(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    names = list(inputs)
    man = str(tmp / "cohort.tsv")
    for tag, opts in (("plain", []), ("uniform", ["-u"]), ("samples", ["-s", str(tmp / "keep.txt")])):
        _cli(["index"] + COMMON + [x for x in opts if x != "-u"] + [fa, vcf, fq])
        singles = _singles(tmp, fa, vcf, inputs, opts)
        assert singles[0] == singles[1] and singles[2] != singles[0] and singles[3] != singles[2]
        texts = {}
        for group in ([], ["--cohort-group", "1"], ["--cohort-group", "3"]):
            d = tmp_path / (tag + "".join(group).strip("-"))
            d.mkdir()
            out = str(d / "merged.vcf")
            assert _cli(["call"] + COMMON + opts + group + ["--cohort", "--merged", out, fa, vcf, man]) == ""
            _no_leftovers(d, ["merged.vcf"])
            texts[tuple(group)] = open(out).read()
            check_paste(texts[tuple(group)], singles, names)
        assert len(set(texts.values())) == 1, "the merged file depends on the grouping"
        merged = texts[()]
        # -o as well: both outputs in one pass, the per-sample files what they were
        for group in ([], ["--cohort-group", "3"]):
            d = tmp_path / (tag + "both" + "".join(group).strip("-"))
            d.mkdir()
            assert _cli(["call"] + COMMON + opts + group + ["--cohort", "-o", str(d / "out"), "--merged", str(d / "m.vcf"), fa, vcf, man]) == ""
            assert open(str(d / "m.vcf")).read() == merged
            assert sorted(os.listdir(d / "out")) == sorted(n + ".vcf" for n in names)
            for n, want in zip(names, singles):
                assert open(str(d / "out" / (n + ".vcf"))).read() == want, n
            _no_leftovers(d, ["m.vcf", "out"])
        # stdout, with the temporary blocks of the groups under $TMPDIR
        for group in ([], ["--cohort-group", "3"]):
            d = tmp_path / (tag + "stdout" + "".join(group).strip("-"))
            d.mkdir()
            assert _cli(["call"] + COMMON + opts + group + ["--cohort", "--merged", "-", fa, vcf, man], env=dict(os.environ, TMPDIR=str(d))) == merged
            _no_leftovers(d, [])
    _no_leftovers(tmp, ["haploid.fq", "dump.txt", "sim1.fq", "sim2.fq", "keep.txt", "cohort.tsv"] + [f for f in os.listdir(tmp) if f.startswith("haploid.vcf.gz")])


def test_cli_merged_verbose_carries_the_coverages(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    names = list(inputs)
    _cli(["index"] + COMMON + [fa, vcf, fq])
    plain_header = _split(_singles(tmp, fa, vcf, {"reads": inputs["reads"]}, [])[0])[0]
    singles = _singles(tmp, fa, vcf, inputs, ["-v"])
    texts = []
    for group in ([], ["--cohort-group", "3"]):
        out = str(tmp_path / ("v" + "".join(group).strip("-") + ".vcf"))
        _cli(["call"] + COMMON + ["-v"] + group + ["--cohort", "--merged", out, fa, vcf, str(tmp / "cohort.tsv")])
        texts.append(open(out).read())
        recs = check_paste(texts[-1], singles, names, plain_header=plain_header)
        assert all(r.split("\t")[7] == "." and r.split("\t")[8] == "GT:GQ:COVS" for r in recs)
    assert texts[0] == texts[1]
    _no_leftovers(tmp_path, ["v.vcf", "vcohort-group3.vcf"])


def test_cli_merged_on_general_blocks(tmp_path):
    """a diploid panel of indel / MNP clusters (tiers 2 and 3, multi-allelic records, a/b cells), built as
    tests/test_gpu_cohort.py::test_cli_cohort_on_general_blocks_and_the_host_enumerator builds it; once more in batches of 7 records"""
    from test_gpu_cohort import _sample_table
    panel = synth.indel_panel(1_500, seed=21, n_samples=70)
    prefix = str(tmp_path / "p")
    synth.write_vcf_fasta(panel, prefix)
    k, ref_k = 35, 43
    names = []
    for s in range(3):
        hi, lo, cnt = _sample_table(synth.flat_kmer_table(panel, 60_000, k, ref_k, seed=5, max_records=1_200), s)
        rows = synth.unpack_ascii(hi, lo, ref_k)
        with open(str(tmp_path / ("s%d.txt" % s)), "w") as fh:
            for r, c in zip(rows, cnt):
                fh.write("%s\t%d\n" % (bytes(r[:ref_k]).decode(), int(c)))
        names.append("s%d" % s)
    (tmp_path / "cohort.tsv").write_text("".join("%s\t%s\n" % (n, n) for n in names))
    common = ["-k", str(k), "-r", str(ref_k), "-b", "1", prefix + ".fa", prefix + ".vcf"]
    env0 = dict(os.environ, MALVA_GENO_BF_BITS=str(1 << 26), MALVA_GENO_BATCH="400")
    _cli(["index"] + common + [str(tmp_path / "s0")], env=env0)
    singles = [_cli(["call"] + common + [str(tmp_path / n)], env=env0) for n in names]
    texts = []
    for batch in ("400", "7"):
        env = dict(env0, MALVA_GENO_BATCH=batch)
        for group in ([], ["--cohort-group", "2"]):
            out = str(tmp_path / ("m%s%s.vcf" % (batch, "".join(group).strip("-"))))
            _cli(["call", "--cohort"] + group + ["--merged", out] + common + [str(tmp_path / "cohort.tsv")], env=env)
            texts.append(open(out).read())
            recs = check_paste(texts[-1], singles, names)
    assert len(set(texts)) == 1
    cells = [c for r in recs for c in r.split("\t")[9:]]
    assert any(not c.startswith("0/0") for c in cells) and any(c.split(":")[0].split("/")[0] != c.split(":")[0].split("/")[1] for c in cells)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".part")]
