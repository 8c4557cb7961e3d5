"""The device k-mer counter (mg_reads_*) against the exact count of the same bytes (oracle/kmc_standin.count_chunks) at its
edges: every (k, ref_k) instantiation of the window kernel, both sides of the 64-bit word, count thresholds, every byte
outside ACGTacgt, chunk lengths around 32-base words, the three paths of reads_reduce_kernel, device input, key partitions,
the call order, and the CLI's carry of a record longer than a chunk.

With the gate off (option use_summary = 0) every ACGT window survives, so the export must equal the exact table; with it
on, the export must hold every row the scan would act on and the counters must equal the CPU oracle's scan of the exact
table."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import vcf_synth
from gpu_util import build_index_pair, map_values_by_key, pad_rows
from malva_amd import BF_ALT, Context, MalvaError, synth
from oracle import capi as ocapi
from oracle import kmc_standin
from test_gpu_reads import BIN, random_reads, run_cli, write_dump

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE = -1, -3
BITS = (1 << 18) + 77          # small filters: many rows hit them, so the gate-on checks have rows to act on
NO_CAP = 2 ** 32 - 1
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _acgt(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()


def _rc(s):
    return s.translate(COMP)[::-1]


def _reads(panel, ref_k, seed, n=2500):
    """reads of the panel's genome (ALT bases at half of the sites) with some N, lower case, reads shorter than ref_k, and
    reverse-complement palindromes (for an even ref_k, windows that are their own reverse complement)"""
    rng = np.random.default_rng(seed)
    out = []
    for s in random_reads(panel.genome, panel, rng, n, lo=max(1, ref_k // 2), hi=ref_k + 200):
        s = bytearray(s)
        if rng.random() < 0.05:
            s[int(rng.integers(0, len(s)))] = ord("N")
        if rng.random() < 0.1:
            a = int(rng.integers(0, len(s)))
            s[a:] = s[a:].lower()
        out.append(bytes(s))
    for _ in range(40):
        h = _acgt(rng, ref_k // 2 + int(rng.integers(0, 4)))
        out += [h + _rc(h)] * int(rng.integers(1, 5))
    return [out[i] for i in rng.permutation(len(out))]


def _chunks(reads, rng, most=60000):
    """whole records, '\\n' after each, cut into chunks of up to about `most` bytes"""
    out, cur, size, want = [], [], 0, int(rng.integers(1, most))
    for r in reads:
        cur.append(r)
        size += len(r) + 1
        if size >= want:
            out.append(b"\n".join(cur) + b"\n")
            cur, size, want = [], 0, int(rng.integers(1, most))
    if cur:
        out.append(b"\n".join(cur) + b"\n")
    return out


def _rows(hi, lo, cnt):
    return dict(zip(zip(hi.tolist(), lo.tolist()), cnt.tolist()))


def _exact(chunks, ref_k, ci=1, cs=NO_CAP):
    """-> ({(hi, lo): count}, ACGT windows, (hi, lo, cnt))"""
    hi, lo, cnt, n_windows = kmc_standin.count_chunks(chunks, ref_k, ci, cs)
    return _rows(hi, lo, cnt), n_windows, (hi, lo, cnt)


def _index(k, ref_k, panel, gate=True, **opts):
    """a device context and the CPU oracle's filters of the same index"""
    ctx = Context(k, ref_k, BITS, device=0)
    if not gate:
        ctx.set_option("use_summary", 0)
    for name, v in opts.items():
        ctx.set_option(name, v)
    return ctx, build_index_pair(ctx, panel, k, ref_k, BITS)


def _export(ctx):
    """-> ({(hi, lo): count} of the export, counts_out of mg_reads_stats)"""
    hi, lo, cnt = ctx.reads_export()
    _, counts = ctx.reads_stats()
    got = _rows(hi, lo, cnt)
    assert len(got) == len(hi) == counts[4]                         # no key twice
    return got, counts


def _count(ctx, chunks, ci, cs, part=0, n_parts=1):
    ctx.reads_begin(ci, cs, part, n_parts)
    for c in chunks:
        ctx.reads_add(c)
    n_kept = ctx.reads_finish()
    got, counts = _export(ctx)
    assert n_kept == len(got)
    return got, counts


def _oracle_counters(oracle, table, k, ref_k):
    """the CPU oracle's scan of a table: (bf counters, map values by key)"""
    obf, octx, omap = oracle
    hi, lo, cnt = table
    ocapi.kmc_scan_packed(octx, obf, omap, hi, lo, cnt, k, ref_k)
    return obf.counts().copy(), dict(omap.items())


def _device_counters(ctx):
    _, _, _, counts = ctx.bf_export(BF_ALT)
    return counts, map_values_by_key(ctx)


def _assert_counters(ctx, want):
    counts, vals = _device_counters(ctx)
    assert np.array_equal(counts, want[0])
    assert vals == want[1]


# ---- a. shapes: both specialised instantiations of reads_window_kernel (35/43, 35/63) and the generic one; ref_k on both sides
# of the 64-bit word (32 / 33), the full 128 bits (64), even ref_k (palindromic windows), k = ref_k, and k < 17 (XXH3's short
# branches)
SHAPES = [(35, 43), (35, 63), (33, 64), (31, 33), (31, 32), (21, 22), (16, 24), (17, 17), (9, 9)]


@pytest.mark.parametrize("k,ref_k", SHAPES)
def test_shape_exact_count(k, ref_k):
    panel = synth.snp_panel(400, seed=200 + ref_k)
    chunks = _chunks(_reads(panel, ref_k, seed=300 + ref_k), np.random.default_rng(ref_k))
    n_bytes = sum(len(c) for c in chunks)
    want, n_windows, table = _exact(chunks, ref_k)
    assert n_windows > 100000
    if ref_k % 2 == 0:
        rows = kmc_standin.decode_m(table[0], table[1], ref_k)
        assert (rows == np.frombuffer(bytes(range(256)).translate(COMP), dtype=np.uint8)[rows[:, ::-1]]).all(axis=1).sum() >= 40

    # gate off: every ACGT window survives, the export is the exact table
    ctx, oracle = _index(k, ref_k, panel, gate=False)
    got, counts = _count(ctx, chunks, 1, NO_CAP)
    assert got == want
    assert counts[0] == n_bytes and counts[1] == n_windows and counts[2] == n_windows and counts[4] == len(want)
    _assert_counters(ctx, _oracle_counters(oracle, table, k, ref_k))
    ctx.close()

    # gate on: the counters of the exact table; the export a subset of it holding every row scan_one acts on
    want2, _, table2 = _exact(chunks, ref_k, 2, 255)
    ctx, oracle = _index(k, ref_k, panel)
    got, counts = _count(ctx, chunks, 2, 255)
    _assert_counters(ctx, _oracle_counters(oracle, table2, k, ref_k))
    assert all(want2.get(key) == c for key, c in got.items())
    obf, _, omap = oracle
    off = (ref_k - k) // 2
    acted = 0
    for key, row in zip(zip(table2[0].tolist(), table2[1].tolist()), kmc_standin.decode_m(table2[0], table2[1], ref_k)):
        centre = row[off:off + k].tobytes()                         # oracle/malva_oracle.c scan_one's cut
        if omap.test_key(centre) or obf.test_key(centre):
            acted += 1
            assert key in got, centre
    assert acted >= 50
    assert counts[0] == n_bytes and counts[1] == n_windows and counts[4] <= counts[2] <= counts[1]
    ctx.close()


# ---- b. count thresholds: k-mers seen exactly ci - 1, ci, ci + 1, cs - 1, cs, cs + 1 times
@pytest.mark.parametrize("ci,cs", [(1, 1), (0, 0), (2, 255), (3, 4), (1, NO_CAP)])
def test_count_thresholds(ci, cs):
    k, ref_k = 35, 43
    panel = synth.snp_panel(300, seed=7)
    rng = np.random.default_rng(1000 + ci * 7 + cs % 1009)
    lo_, hi_ = max(ci, 1), max(cs, 1)                               # (0 reads as 1, both)
    times = [0, 1, 2, 70000] if cs == NO_CAP else [lo_ - 1, lo_, lo_ + 1, hi_ - 1, hi_, hi_ + 1]
    planted, recs = [], []
    for t in times:
        w = _acgt(rng, ref_k)
        planted.append((w, t))
        for _ in range(t):                                          # either strand, some of it in lower case
            s = w if rng.random() < 0.5 else _rc(w)
            recs.append(s.lower() if rng.random() < 0.2 else s)
    recs += random_reads(panel.genome, panel, rng, 800)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    chunks = _chunks(recs, rng, most=200000)
    want, _, _ = _exact(chunks, ref_k, lo_, hi_)
    ctx, _ = _index(k, ref_k, panel, gate=False)
    got, _ = _count(ctx, chunks, ci, cs)
    assert got == want
    for w, t in planted:
        h, l, _, _ = kmc_standin.count_chunks([w], ref_k)
        key = (int(h[0]), int(l[0]))
        assert got.get(key) == (min(t, hi_) if t >= lo_ else None), t
    if cs == NO_CAP:
        assert 70000 in got.values()
    ctx.close()


# ---- c. bytes and chunk lengths
def _byte_records(rng, ref_k):
    r = ref_k
    recs = [b"", b"", _acgt(rng, 1), _acgt(rng, r - 1), _acgt(rng, r), _acgt(rng, r + 1), b"", _acgt(rng, r + 1).lower()]
    for b in range(256):
        if bytes([b]) in b"ACGTacgt":
            continue
        x = bytes([b])
        recs.append(_acgt(rng, r) + x + _acgt(rng, r))              # the last base of window 1, the first of window r
        recs.append(x + _acgt(rng, r) + x)                          # the first and last base of a record
        m = _acgt(rng, r)
        recs.append(m[:r // 2] + x + m[r // 2 + 1:])                # the middle of the record's only window
    for _ in range(600):                                            # mixed case, base by base
        s = bytearray(_acgt(rng, int(rng.integers(r, 4 * r))))
        for p in np.nonzero(rng.random(len(s)) < 0.3)[0]:
            s[p] |= 0x20
        recs.append(bytes(s))
    return [recs[i] for i in rng.permutation(len(recs))]


def _cut(stream, sizes):
    out, at, i = [], 0, 0
    while at < len(stream):
        out.append(stream[at:at + sizes[i % len(sizes)]])
        at += sizes[i % len(sizes)]
        i += 1
    return out


@pytest.mark.parametrize("k,ref_k", [(35, 43), (33, 64)])
def test_bytes_and_chunk_edges(k, ref_k):
    rng = np.random.default_rng(40 + ref_k)
    panel = synth.snp_panel(300, seed=11)
    stream = b"\n".join(_byte_records(rng, ref_k)) + b"\n"
    r = ref_k
    sizes = [1, r - 1, r, r + 1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 30000]
    ctx, _ = _index(k, ref_k, panel, gate=False)
    for phase in (0, 5):                                            # the same lengths at other offsets of the stream
        chunks = _cut(stream, sizes[phase:] + sizes[:phase])
        assert b"".join(chunks) == stream
        want, n_windows, _ = _exact(chunks, ref_k)
        ctx.reads_begin(1, NO_CAP)
        ctx.reads_add(b"")
        for c in chunks:
            ctx.reads_add(c)
        ctx.reads_add(b"")
        assert ctx.reads_finish() == len(want)
        got, counts = _export(ctx)
        assert got == want
        assert counts[0] == len(stream) and counts[1] == counts[2] == n_windows
    # nothing but chunks that hold no window
    ctx.reads_begin(1, NO_CAP)
    for c in (b"", _acgt(rng, r - 1), b"N" * 300, b"\n", _acgt(rng, r - 1) + b"\x00" + _acgt(rng, r - 1)):
        ctx.reads_add(c)
    assert ctx.reads_finish() == 0
    got, counts = _export(ctx)
    assert got == {} and counts[1] == counts[2] == counts[4] == 0
    ctx.close()


# ---- d. the three paths of reads_reduce_kernel, in one bin (reads_parts_log2 = 0) with the gate off, so that the bin's size and
# distinct keys are known on the host
def _reduce_inputs(panel, ref_k, rng):
    # tiles only: 40 reads of 100 bases, 2,320 windows <= RD_TILE (4,096 pairs): the bin is reduced in LDS at once
    tiles = [panel.genome[p:p + 100].tobytes() for p in rng.integers(0, len(panel.genome) - 100, size=40)]
    # shrink, then LDS: 40 distinct windows, 500 copies each (20,000 pairs, 5 tiles): a tile round leaves at most 200
    # pairs, far below three quarters of the bin, and the 200 then fit one tile
    keys = [_acgt(rng, ref_k) for _ in range(40)]
    shrink = [w if rng.random() < 0.5 else _rc(w) for w in keys for _ in range(500)]
    # global sort: 20,000 distinct windows, 8 copies each, shuffled (160,000 pairs, 40 tiles): a tile of 4,096 pairs holds
    # about 3,750 distinct keys, so the round shrinks the bin by ~8 %, not by a quarter, and the bin (counts now 1 or 2 and
    # more) is sorted in global memory and its runs added
    keys = [_acgt(rng, ref_k) for _ in range(20000)]
    glob = [w if rng.random() < 0.5 else _rc(w) for w in keys for _ in range(8)]
    return {"tiles": tiles, "shrink": shrink, "global": glob}


def test_reduce_paths_one_bin():
    k, ref_k = 35, 43
    panel = synth.snp_panel(300, seed=19)
    rng = np.random.default_rng(20)
    inputs = _reduce_inputs(panel, ref_k, rng)
    ctx, _ = _index(k, ref_k, panel, gate=False, reads_parts_log2=0)
    for name, recs in inputs.items():
        recs = [recs[i] for i in rng.permutation(len(recs))]
        chunks = _chunks(recs, rng, most=400000)
        want, n_windows, _ = _exact(chunks, ref_k)
        assert (n_windows <= 4096) == (name == "tiles") and len(want) == {"tiles": len(want), "shrink": 40, "global": 20000}[name]
        for opts in ({"reads_passes": 1, "reads_budget_mb": 4096}, {"reads_passes": 3, "reads_budget_mb": 1}):
            for o, v in opts.items():
                ctx.set_option(o, v)
            got, counts = _count(ctx, chunks, 1, NO_CAP)
            assert got == want, (name, opts)
            assert counts[1] == counts[2] == n_windows
    ctx.close()


# ---- e. device input (gate off): mg_reads_add_device from an aligned buffer (packed in place) and at offsets 1..3 (copied into
# a staging slot), and host and device chunks alternated
def test_device_input_paths():
    k, ref_k = 35, 43
    panel = synth.snp_panel(400, seed=23)
    rng = np.random.default_rng(24)
    reads = _reads(panel, ref_k, seed=25)
    chunks = _chunks(reads, rng)
    i, growing, size = 0, [], 2000                                  # whole records, chunks that grow (both slots reallocated)
    while i < len(reads):
        j = i + 1
        while j < len(reads) and sum(len(r) + 1 for r in reads[i:j]) < size:
            j += 1
        growing.append(b"\n".join(reads[i:j]) + b"\n")
        i, size = j, size * 3 // 2
    want, n_windows, table = _exact(chunks, ref_k, 2, 255)
    assert _exact(growing, ref_k, 2, 255)[0] == want
    results, keep, oracle_counters = [], [], None

    def to_device(c, off):
        t = torch.zeros(len(c) + off + 64, dtype=torch.uint8, device="cuda:0")
        t[off:off + len(c)].copy_(torch.frombuffer(bytearray(c), dtype=torch.uint8))
        keep.append(t)                                              # alive and unchanged until reads_finish returns
        ptr = t.data_ptr() + off
        assert (ptr & 3 == 0) == (off == 0)
        return ptr

    plans = [("host", chunks, [None]), ("aligned", chunks, [0]), ("offset 1", chunks, [1]), ("offset 2", chunks, [2]),
             ("offset 3", chunks, [3]), ("mixed", growing, [None, 1, 0, None, None, 3, 2, 0, None, 1])]
    for name, cs, offs in plans:
        ctx, oracle = _index(k, ref_k, panel, gate=False)
        if oracle_counters is None:
            oracle_counters = _oracle_counters(oracle, table, k, ref_k)
        ctx.reads_begin(2, 255)
        ptrs = [None if offs[n % len(offs)] is None else to_device(c, offs[n % len(offs)]) for n, c in enumerate(cs)]
        empty = to_device(b"ACGT", 0)
        torch.cuda.synchronize()                                    # the tensors' writes ordered before the calls
        if name != "host":
            ctx.reads_add_device(empty, 0)                          # an empty device chunk
        for c, p in zip(cs, ptrs):
            if p is None:
                ctx.reads_add(c)
            else:
                ctx.reads_add_device(p, len(c))
        ctx.reads_finish()
        keep.clear()
        got, counts = _export(ctx)
        assert got == want, name
        assert counts[0] == sum(len(c) for c in cs) and counts[1] == counts[2] == n_windows, name
        _assert_counters(ctx, oracle_counters)
        results.append((got, counts[1:], _device_counters(ctx)))
        ctx.close()
    for got, counts, dev in results[1:]:
        assert got == results[0][0] and counts == results[0][1]
        assert np.array_equal(dev[0], results[0][2][0]) and dev[1] == results[0][2][1]


# ---- f. key partitions on one device
def test_partitions_are_disjoint_and_sum():
    k, ref_k = 35, 43
    panel = synth.snp_panel(400, seed=29)
    chunks = _chunks(_reads(panel, ref_k, seed=30), np.random.default_rng(31))
    for gate in (False, True):
        ctx, _ = _index(k, ref_k, panel, gate=gate)
        whole, counts = _count(ctx, chunks, 2, 255)
        whole_counters = _device_counters(ctx)
        ctx.close()
        if not gate:
            assert whole == _exact(chunks, ref_k, 2, 255)[0]
        parts, bf_sum, map_sum = [], np.zeros(len(whole_counters[0]), dtype=np.uint32), {}
        for p in range(3):
            ctx, _ = _index(k, ref_k, panel, gate=gate)
            got, pc = _count(ctx, chunks, 2, 255, part=p, n_parts=3)
            assert pc[1] == counts[1]                               # every part sees every window ...
            parts.append(got)                                       # ... and keeps its own keys
            bf, vals = _device_counters(ctx)
            bf_sum += bf.astype(np.uint32)
            for key, v in vals.items():
                map_sum[key] = (map_sum.get(key, 0) + v) & 0xFFFFFFFF
            ctx.close()
        assert all(len(x) > 0 for x in parts)
        for a in range(3):
            for b in range(a + 1, 3):
                assert not set(parts[a]) & set(parts[b])
        union = {}
        for x in parts:
            union.update(x)
        assert union == whole
        assert np.array_equal(bf_sum & 0xFFFF, whole_counters[0].astype(np.uint32))
        assert map_sum == {key: v & 0xFFFFFFFF for key, v in whole_counters[1].items()}


# ---- g. call order and arguments
def _code(call):
    with pytest.raises(MalvaError) as e:
        call()
    return e.value.code


def test_call_order_and_arguments():
    k, ref_k = 35, 43
    panel = synth.snp_panel(300, seed=37)
    chunks = _chunks(_reads(panel, ref_k, seed=38, n=1500), np.random.default_rng(39))
    other = _chunks(_reads(panel, ref_k, seed=40, n=1500), np.random.default_rng(41))
    fresh = Context(k, ref_k, BITS, device=0)
    for call in (lambda: fresh.reads_add(b"ACGT" * 20), fresh.reads_finish, fresh.reads_export, fresh.reads_stats):
        assert _code(call) == MG_ERR_STATE
    assert _code(lambda: fresh.reads_begin(1, 255)) == MG_ERR_STATE  # neither filter finalised
    rows, valid = synth.signature_rows(panel, k)
    fresh.bf_insert(BF_ALT, pad_rows(rows[valid]))
    fresh.bf_finalize(BF_ALT)
    assert _code(lambda: fresh.reads_begin(1, 255)) == MG_ERR_STATE  # the context filter not finalised
    fresh.close()
    ctx, _ = _index(k, ref_k, panel, reads_passes=3)
    for part, n_parts in ((3, 3), (0, 0), (5, 2)):
        assert _code(lambda: ctx.reads_begin(1, 255, part, n_parts)) == MG_ERR_ARG
    ctx.reads_begin(2, 255)
    assert _code(ctx.reads_export) == MG_ERR_STATE and _code(ctx.reads_stats) == MG_ERR_STATE
    for c in chunks:
        ctx.reads_add(c)
    n = ctx.reads_finish()
    assert n > 10
    assert _code(lambda: ctx.reads_add(b"ACGT" * 20)) == MG_ERR_STATE and _code(ctx.reads_finish) == MG_ERR_STATE
    hi, lo, cnt = ctx.reads_export()
    for cap in (0, 1, n // 2, n - 1, n, n + 5):                     # the first cap rows; *n_out = all of them
        h, l_, c, total = ctx.reads_export(cap, with_total=True)
        m = min(cap, n)
        assert total == n and len(h) == m
        assert np.array_equal(h, hi[:m]) and np.array_equal(l_, lo[:m]) and np.array_equal(c, cnt[:m])
    # a second begin starts a fresh count
    ctx.reads_begin(2, 255)
    for c in other:
        ctx.reads_add(c)
    ctx.reads_finish()
    again, _ = _export(ctx)
    ctx.close()
    ctx, _ = _index(k, ref_k, panel, reads_passes=3)
    want, _ = _count(ctx, other, 2, 255)
    ctx.close()
    assert again == want and again != _rows(hi, lo, cnt)


# ---- 4. the CLI's carry: a FASTA record longer than a chunk continues in the next one behind its last ref_k - 1 bases
CHUNK = 8192


def _donors(contigs, records, rng):
    """both haplotypes of a donor that carries a random allele of every record"""
    out = []
    for _ in range(2):
        for name, seq in contigs.items():
            parts, last = [], 0
            for (cn, pos, ref, alts) in records:
                real = [a for a in alts if not a.startswith("<")]
                if cn != name or pos < last:
                    continue
                pick = int(rng.integers(0, len(real) + 1))
                parts.append(seq[last:pos])
                parts.append(ref if pick == 0 else real[pick - 1])
                last = pos + len(ref)
            parts.append(seq[last:])
            out.append("".join(parts).encode())
    return out


def _run_cli_err(args, env):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    m = re.search(r"\[malva-geno\] counted (\d+) (\d+)-mer windows", r.stderr)
    assert m, r.stderr[-3000:]
    return r.stdout, int(m.group(1))


@pytest.mark.parametrize("k,ref_k", [(35, 43), (35, 63)])
def test_cli_long_fasta_records_carry(tmp_path, k, ref_k):
    prefix = str(tmp_path / "case")
    contigs, records = vcf_synth.make_case(prefix, 70 + ref_k, n_clusters=400, k=k, vcf_strip_chr=True)
    rng = np.random.default_rng(ref_k)
    donors = _donors(contigs, records, rng)
    d0 = donors[0]
    # the chunker's edges first, from an empty chunk: a record of chunk - 1 bases fills it to the byte; a short record and one
    # that ends exactly where the room runs out; a record of chunk bases (a carry with one base behind it)
    recs = [d0[:CHUNK - 1], d0[100:200], d0[300:300 + CHUNK - 1 - 101], d0[1000:1000 + CHUNK]]
    for d in donors:                                                # then records of 30k .. 100k bases
        if len(d) >= 30000:
            recs.append(d[:100000])
        for _ in range(2):
            L = int(rng.integers(30000, min(len(d), 100000) + 1))
            a = int(rng.integers(0, len(d) - L + 1))
            recs.append(d[a:a + L])
    fa = str(tmp_path / "reads.fa")
    with open(fa, "wb") as fh:
        for i, s in enumerate(recs):
            w = 60 + i % 17
            fh.write(b">c%d\n" % i + b"".join(s[j:j + w] + b"\n" for j in range(0, len(s), w)) + b"\n" * (i % 3 == 1))
    assert kmc_standin.read_fasta(fa) == recs
    gz = fa + ".gz"
    with open(fa, "rb") as a, gzip.open(gz, "wb") as b:
        b.write(a.read())
    hi, lo, cnt, n_windows = kmc_standin.count_chunks(recs, ref_k)
    kmers = [r.tobytes() for r in kmc_standin.decode_m(hi, lo, ref_k)]
    args = ["-k", str(k), "-r", str(ref_k), "-b", "1", "-p", prefix + ".fa", prefix + ".vcf"]
    run_cli(["index"] + args + [fa])
    env = dict(os.environ, MALVA_GENO_READS_CHUNK=str(CHUNK))
    for ci, cs in ((1, 255), (2, 255)):
        dump = str(tmp_path / ("dump_%d_%d.txt" % (ci, cs)))
        write_dump(dump, [(km, min(int(c), cs)) for km, c in zip(kmers, cnt) if c >= ci])
        want = run_cli(["call"] + args + [dump])
        assert sum(1 for l in want.split("\n") if l and not l.startswith("#")) > 100
        opt = ["--min-count", str(ci), "--max-count", str(cs)]
        runs = [(fa, env)]
        if (ci, cs) == (2, 255):
            runs += [(gz, env), (fa, dict(env, MALVA_GENO_SHARE_DEVICE="1"))]
        for n, (path, e) in enumerate(runs):
            gpus = ["--gpus", "2"] if n == 2 else []
            got, counted = _run_cli_err(["call"] + gpus + opt + args + [path], e)
            assert counted == n_windows, (ci, cs, path, gpus)          # a carry of the wrong length shows here
            assert got == want, (ci, cs, path, gpus)
