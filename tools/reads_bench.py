"""Counting from reads on one MI355X (mg_reads_*): a C3-like index (synth.snp_panel, 1e6 SNPs, k35 r43 b4) and synthetic 150-nt
reads of its donor (the panel's ALT base at half of the sites) at 10x.  Prints one JSON line: device ms per phase (HIP events,
mg_reads_stats), bases/s and windows/s, the gate's pass fraction, passes, k-mers kept, a parity bit (the counters after
mg_reads_* against mg_kmc_scan of the exact table of a subsample, counted here with numpy), and -- with --cli -- the wall time of
`malva-geno call` on the same reads as .fq and as .fq.gz, with its MALVA_GENO_TIMERS lines.

    python tools/reads_bench.py [--snps 1000000] [--coverage 10] [--parity-reads 100000] [--cli]
"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (the first HIP runtime in the process, as in bench.py)
except ImportError:
    pass
from malva_amd import BF_ALT, BF_CTX, Context, synth  # noqa: E402

K, REF_K, READ_LEN = 35, 43, 150
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def build_index(panel, bits):
    ctx = Context(K, REF_K, bits, device=0)
    sig, valid = synth.snp_signature_rows(panel, K)
    rows = np.zeros((sig.shape[0], 40), dtype=np.uint8)
    rows[:, :K] = sig
    ctx.map_insert(rows[0::2][valid[0::2]])
    ctx.bf_insert(BF_ALT, rows[1::2][valid[1::2]])
    ctx.bf_finalize(BF_ALT)
    ctx.ref_scan(panel.genome.tobytes())
    ctx.bf_finalize(BF_CTX)
    return ctx


def donor_of(panel, seed):
    g = panel.genome.copy()
    alts = panel.pool[panel.allele_off[panel.var_allele_off[:-1] + 1]]
    take = np.random.default_rng(seed).random(panel.n) < 0.5
    g[panel.pos[take]] = alts[take]
    return g


def read_batches(donor, n_reads, seed, batch=400_000):
    """(batch, READ_LEN + 1) uint8 arrays: reads of the donor, each ending in '\\n'"""
    rng = np.random.default_rng(seed)
    ar = np.arange(READ_LEN, dtype=np.int64)
    for b0 in range(0, n_reads, batch):
        nb = min(batch, n_reads - b0)
        starts = rng.integers(0, len(donor) - READ_LEN, size=nb)
        out = np.empty((nb, READ_LEN + 1), dtype=np.uint8)
        out[:, :READ_LEN] = donor[starts[:, None] + ar]
        out[:, READ_LEN] = 10
        yield out


def exact_table(batch, ci=2, cs=255):
    """KMC's table of these reads (canonical 43-mers, count >= ci, capped at cs) as SoA (hi, lo, cnt)"""
    lut = np.zeros(256, dtype=np.uint64)
    lut[ACGT] = np.arange(4, dtype=np.uint64)
    codes = lut[batch[:, :READ_LEN]]
    nw = READ_LEN - REF_K + 1

    def halves(c):  # first 21 bases (42 bits), last 22 bases (44 bits) of every window, M-form
        a = np.zeros((c.shape[0], nw), dtype=np.uint64)
        b = np.zeros((c.shape[0], nw), dtype=np.uint64)
        for j in range(21):
            a = (a << np.uint64(2)) | c[:, j:j + nw]
        for j in range(21, REF_K):
            b = (b << np.uint64(2)) | c[:, j:j + nw]
        return a.reshape(-1), b.reshape(-1)

    fa, fb = halves(codes)
    rc = (np.uint64(3) - codes)[:, ::-1]
    ra, rb = halves(rc)
    ra = ra.reshape(-1, nw)[:, ::-1].reshape(-1)   # (window p of the read = window nw-1-p of its reverse complement)
    rb = rb.reshape(-1, nw)[:, ::-1].reshape(-1)
    take_f = (fa < ra) | ((fa == ra) & (fb <= rb))
    a = np.where(take_f, fa, ra)
    b = np.where(take_f, fb, rb)
    key = np.stack([a, b], axis=1)
    uk, cnt = np.unique(key, axis=0, return_counts=True)
    keep = cnt >= ci
    uk, cnt = uk[keep], np.minimum(cnt[keep], cs).astype(np.uint32)
    hi = uk[:, 0] >> np.uint64(20)
    lo = ((uk[:, 0] & np.uint64((1 << 20) - 1)) << np.uint64(44)) | uk[:, 1]
    return hi, lo, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--coverage", type=float, default=10.0)
    ap.add_argument("--parity-reads", type=int, default=100_000)
    ap.add_argument("--cli", action="store_true")
    a = ap.parse_args()
    bits = 4 << 33
    panel = synth.snp_panel(a.snps, seed=20261016)
    donor = donor_of(panel, 1)
    n_reads = int(len(donor) * a.coverage / READ_LEN)
    out = {"workload": "reads_count", "snps": a.snps, "genome_bases": int(len(donor)), "reads": n_reads, "read_len": READ_LEN,
           "coverage": a.coverage, "k": K, "ref_k": REF_K, "bf_bits": bits}

    # the device path on the full read set, fed from host memory in 64 MiB chunks
    ctx = build_index(panel, bits)
    batches = list(read_batches(donor, n_reads, 2))
    ctx.reads_begin(2, 255)
    ctx.synchronize()
    t0 = time.perf_counter()
    for b in batches:
        flat = b.reshape(-1)
        step = (64 << 20) // (READ_LEN + 1) * (READ_LEN + 1)
        for i in range(0, flat.size, step):
            ctx.reads_add(flat[i:i + step].tobytes())
    t_add = time.perf_counter() - t0
    kept = ctx.reads_finish()
    wall = time.perf_counter() - t0
    ms, counts = ctx.reads_stats()
    dev_ms = sum(ms)
    out.update({"ms": {"pack": round(ms[0], 3), "window_filter": round(ms[1], 3), "file": round(ms[2], 3), "reduce": round(ms[3], 3),
                       "scan": round(ms[4], 3), "device_total": round(dev_ms, 3)},
                "host_wall_s": round(wall, 3), "host_add_s": round(t_add, 3),
                "bases": int(counts[0]), "windows": int(counts[1]), "survivors": int(counts[2]), "passes": int(counts[3]), "kept": int(counts[4]),
                "gate_pass_fraction": round(counts[2] / max(1, counts[1]), 4),
                "bases_per_s_device": float("%.4g" % (counts[0] / (dev_ms / 1e3))), "windows_per_s_device": float("%.4g" % (counts[1] / (dev_ms / 1e3))),
                "bases_per_s_wall": float("%.4g" % (counts[0] / wall))})
    ctx.close()

    # parity on a subsample: counters after mg_reads_* == counters after mg_kmc_scan of the exact table
    sub = batches[0][:a.parity_reads]
    hi, lo, cnt = exact_table(sub)
    c1, c2 = build_index(panel, bits), build_index(panel, bits)
    c1.kmc_scan(hi, lo, cnt)
    c2.reads_begin(2, 255)
    c2.reads_add(sub.reshape(-1).tobytes())
    c2.reads_finish()
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(c1.bf_export(BF_ALT), c2.bf_export(BF_ALT)))
    k1, v1 = c1.map_export()
    k2, v2 = c2.map_export()
    same = same and dict(zip(k1, v1.tolist())) == dict(zip(k2, v2.tolist()))
    out["parity"] = {"reads": int(sub.shape[0]), "table_rows": int(len(hi)), "counters_equal": bool(same)}
    c1.close()
    c2.close()

    if a.cli:
        binp = os.path.join(ROOT, "bin", "malva-geno")
        with tempfile.TemporaryDirectory() as td:
            prefix = os.path.join(td, "c3")
            synth.write_vcf_fasta(synth.flat_from_snp_panel(panel), prefix)
            fq = os.path.join(td, "reads.fq")
            with open(fq, "wb") as fh, gzip.open(fq + ".gz", "wb", compresslevel=1) as gz:
                for b in batches:
                    n = b.shape[0]
                    rec = np.empty((n, 3 + (READ_LEN + 1) + 2 + (READ_LEN + 1)), dtype=np.uint8)   # @r / sequence / + / quality
                    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
                    rec[:, 3:4 + READ_LEN] = b
                    rec[:, 4 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"+\n", dtype=np.uint8)
                    rec[:, 6 + READ_LEN:-1] = ord("I")
                    rec[:, -1] = 10
                    data = rec.tobytes()
                    fh.write(data)
                    gz.write(data)
            common = ["-k", str(K), "-r", str(REF_K), "-b", "4", prefix + ".fa", prefix + ".vcf"]
            subprocess.run([binp, "index"] + common + [fq], check=True, capture_output=True, timeout=1200)
            env = dict(os.environ, MALVA_GENO_TIMERS="1")
            for name, path in (("fq", fq), ("fq_gz", fq + ".gz")):
                t0 = time.perf_counter()
                r = subprocess.run([binp, "call"] + common + [path], capture_output=True, text=True, timeout=1800, env=env)
                w = time.perf_counter() - t0
                timers = [l.split("]", 1)[1].strip() for l in r.stderr.split("\n") if "timer]" in l and ("reads" in l or "table scan" in l)]
                out["cli_" + name] = {"rc": r.returncode, "wall_s": round(w, 2), "bytes": os.path.getsize(path), "timers": timers}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
