"""The kernels behind `call --cohort --site-stats` on one MI355X, through the C ABI.

Counts leg: mg_site_geno_counts on 64 planes x 1e6 records -- records of 2 alleles with a few of 3 and 4, calls drawn at a skewed allele
frequency with a few indexes outside the record, GQ on both sides of the mask.  Reported: the device milliseconds of a call (mg_hwe_stats:
the kernel alone, no copy), the median of --repeats calls with their spread; the bytes it must move -- 12 B per cell (gt1, gt2, gq), 8 B
per record of var_allele_off, 4 B per record and 8 B per allele slot written -- and the time those take at half the HBM rate of 8 TB/s,
which is the expectation to hold the measurement against.  The counts are compared with tests/site_stats_model.py, all of them.
Test leg: mg_hwe_exact on that run's biallelic items (one per record of 2 alleles).
Wide leg: mg_hwe_exact on --wide-items items of n = 16,384 individuals in Hardy-Weinberg proportions, allele frequencies spread evenly
over (0, 0.5]: r / 2 steps of one f64 division per walk, up to 8,192.
Beside each of the two, the same loop in C++ on one host core (tools/site_stats_host_loop.cpp, built here with -O2 -ffp-contract=off and
timed here): on all items of the test leg, on --host-wide-items evenly spaced items of the wide leg, scaled to all of them.  The host's
doubles are compared with the device's bit for bit.  No ratio is promised.

    python tools/site_stats_bench.py [--planes 64] [--records 1000000] [--repeats 5] [--out profiles/site_stats_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from malva_amd import Context  # noqa: E402
from site_stats_model import geno_counts_plain  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def host_loop(directory):
    so = os.path.join(directory, "site_stats_host_loop.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "site_stats_host_loop.cpp")], check=True)
    f = C.CDLL(so).hwe_exact_host
    f.argtypes = [C.c_size_t] + [C.c_void_p] * 5
    f.restype = None

    def run(n, het, hom):
        hwe, exc = np.zeros(n.size), np.zeros(n.size)
        t0 = time.perf_counter()
        f(n.size, *(x.ctypes.data_as(C.c_void_p) for x in (n, het, hom, hwe, exc)))
        return hwe, exc, (time.perf_counter() - t0) * 1e3
    return run


def same_bits(a, b):
    return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-gq", type=int, default=20)
    ap.add_argument("--wide-items", type=int, default=1_000_000)
    ap.add_argument("--host-wide-items", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_stats_bench.json"))
    a = ap.parse_args()
    P, n = a.planes, a.records
    rng = np.random.default_rng(20261020)
    A = rng.choice(np.array([2, 3, 4]), size=n, p=[0.95, 0.04, 0.01])
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)
    slots = int(vao[-1])
    af = rng.beta(0.5, 2.0, size=n)

    def draw():
        g = ((rng.random((P, n)) < af[None, :]) * rng.integers(1, 4, size=(P, n))).astype(np.int32)   # (an index of 2 or 3 in a record of 2 alleles: not usable)
        g[rng.random((P, n)) < 0.01] = -1
        return g
    g1, g2 = draw(), draw()
    gq = rng.integers(0, 120, size=(P, n)).astype(np.int32)
    out = {"workload": "site_stats", "planes": P, "records": n, "allele_slots": slots, "repeats": a.repeats, "min_gq": a.min_gq}
    # the wide leg's items: n individuals at allele frequency p in Hardy-Weinberg proportions
    W, big = a.wide_items, 16384
    p = (np.arange(W, dtype=np.float64) + 1) / W * 0.5
    w_hom = np.floor(big * p * p).astype(np.uint32)
    w_het = np.floor(big * 2 * p * (1 - p)).astype(np.uint32)
    w_n = np.full(W, big, dtype=np.uint32)
    with tempfile.TemporaryDirectory() as tmp, Context(35, 43, 1 << 20) as c:
        host = host_loop(tmp)
        ms = []
        counts = None
        for _ in range(a.repeats + 1):                                       # (the first call allocates: not kept)
            counts = c.site_geno_counts(g1, g2, gq, False, vao, min_gq=a.min_gq)
            ms.append(c.hwe_stats()[0])
        out["count_ms"] = stat(ms[1:])
        step = 100_000
        want = [geno_counts_plain(g1[:, v:v + step], g2[:, v:v + step], gq[:, v:v + step], False, vao[v:min(v + step, n) + 1] - vao[v], a.min_gq) for v in range(0, n, step)]
        out["counts_equal_model"] = int(all(np.array_equal(counts[k], np.concatenate([w[k] for w in want])) for k in range(3)))
        out["usable_cells"] = int(counts[0].sum())
        moved = 12 * P * n + 8 * n + 4 * n + 8 * slots
        out["bytes"] = moved
        out["gb_per_s"] = round(moved / out["count_ms"]["median"] / 1e6, 1)
        out["expected_ms_at_half_hbm"] = round(moved / (HBM_BYTES_PER_S / 2) * 1e3, 4)
        # the test leg: the biallelic records' one item each
        bi = np.flatnonzero(A == 2)
        t_n, t_het, t_hom = (np.ascontiguousarray(x) for x in (counts[0][bi], counts[1][vao[bi] + 1], counts[2][vao[bi] + 1]))
        for tag, (i_n, i_het, i_hom), host_items in (("test", (t_n, t_het, t_hom), t_n.size), ("wide", (w_n, w_het, w_hom), min(a.host_wide_items, W))):
            ms = []
            for _ in range(a.repeats + 1):
                hwe, exc = c.hwe_exact(i_n, i_het, i_hom)
                ms.append(c.hwe_stats()[1])
            pick = np.unique(np.linspace(0, i_n.size - 1, host_items).astype(np.int64)) if i_n.size else np.zeros(0, dtype=np.int64)
            h_hwe, h_exc, h_ms = host(*(np.ascontiguousarray(x[pick]) for x in (i_n, i_het, i_hom)))
            out[tag] = {"items": int(i_n.size), "device_ms": stat(ms[1:]), "host_items": int(pick.size), "host_ms": round(h_ms, 2),
                        "host_ms_scaled_to_all_items": round(h_ms * i_n.size / max(pick.size, 1), 1),
                        "host_equals_device_bits": int(same_bits(h_hwe, hwe[pick]) and same_bits(h_exc, exc[pick])),
                        "hwe_below_1e-6": int((hwe < 1e-6).sum()), "nan": int(np.isnan(hwe).sum())}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
