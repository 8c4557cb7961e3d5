"""The kernel behind `call --cohort --sample-stats` on one MI355X, through the C ABI: mg_sample_counts on 64 planes x 1e6 records --
records of 2 alleles with a few of 3 and 4, calls drawn at a skewed allele frequency with a few indexes outside the record, GQ on
both sides of the mask, coverages, status codes and allele classes on every slot.

Reported: the device milliseconds of a call (mg_sample_stats: the memset and the kernel alone, no copy), the median of --repeats
calls with their spread; the bytes it must move -- 12 B per cell (gt1, gt2, gq), 1 B per cell of status, 4 B per allele slot and
plane of cov, 8 B per record and plane of var_allele_off (every plane's waves read it again) -- and the rate that follows; the time
those bytes take at half the HBM rate of 8 TB/s, which is the expectation to hold the measurement against.  The table is compared
with the numpy restatement of tests/test_sample_stats_cpu.py, all of it.

    python tools/sample_stats_bench.py [--planes 64] [--records 1000000] [--repeats 5] [--out profiles/sample_stats_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from malva_amd import Context  # noqa: E402
from test_sample_stats_cpu import sample_counts_plain  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-gq", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_stats_bench.json"))
    a = ap.parse_args()
    P, n = a.planes, a.records
    rng = np.random.default_rng(20261018)
    A = rng.choice(np.array([2, 3, 4]), size=n, p=[0.95, 0.04, 0.01])
    vao = np.zeros(n + 1, dtype=np.uint32)
    vao[1:] = np.cumsum(A)
    slots = int(vao[-1])
    af = rng.beta(0.5, 2.0, size=n)

    def draw():
        g = ((rng.random((P, n)) < af[None, :]) * rng.integers(1, 4, size=(P, n))).astype(np.int32)   # (an index of 2 or 3 in a record of 2 alleles: BAD)
        g[rng.random((P, n)) < 0.01] = -1
        return g
    g1, g2 = draw(), draw()
    gq = rng.integers(0, 120, size=(P, n)).astype(np.int32)
    status = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3], dtype=np.uint8), size=(P, n))
    cov = rng.integers(0, 200, size=(P, slots)).astype(np.uint32)
    cls = rng.integers(1, 6, size=slots).astype(np.uint8)
    cls[vao[:-1]] = 0
    out = {"workload": "sample_stats", "planes": P, "records": n, "allele_slots": slots, "repeats": a.repeats, "min_gq": a.min_gq}
    with Context(35, 43, 1 << 20) as c:
        ms = []
        counts = None
        for _ in range(a.repeats + 1):                                       # (the first call allocates: not kept)
            counts = c.sample_counts(g1, g2, gq, False, vao, status, cov, cls, min_gq=a.min_gq, counts=counts, overwrite=True)
            ms.append(c.sample_stats())
    want = np.concatenate([sample_counts_plain(g1[p:p + 8], g2[p:p + 8], gq[p:p + 8], False, vao, status[p:p + 8], cov[p:p + 8], cls, a.min_gq)
                           for p in range(0, P, 8)])
    out["counts_equal_numpy"] = int(np.array_equal(counts, want))
    out["called_cells"] = int(counts[:, 3].sum())
    out["count_ms"] = stat(ms[1:])
    moved = 13 * P * n + 4 * P * slots + 8 * P * n
    out["bytes"] = moved
    out["gb_per_s"] = round(moved / out["count_ms"]["median"] / 1e6, 1)
    out["expected_ms_at_half_hbm"] = round(moved / (HBM_BYTES_PER_S / 2) * 1e3, 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
