"""The kernels behind `call --cohort --ld` on one MI355X, through the C ABI's device forms (the tables are made on the device with torch, so
no leg pays a copy).

Pack leg: mg_pack_site_dosage on 64 planes x 1e6 biallelic records -- calls drawn at a skewed allele frequency with a few indexes outside
the record, GQ on both sides of the mask.  Reported: the device milliseconds of a call (mg_ld_stats: the kernel alone), the median of
--repeats calls with their spread; the bytes it must move -- 12 B per cell (gt1, gt2, gq), 8 B per record of var_allele_off, 24 B per
record written -- and the time those take at half the HBM rate of 8 TB/s.  A slice of the words is compared with tests/ld_model.py.
Window legs: mg_ld_window at window 64 (no base limit, min_n 2, min_r2 0.2) on 1e6 records for n_groups 1 and 256: random words -- a cell
contributes in seven of eight cases, dosages 0 / 1 / 2 at about 0.50 / 0.33 / 0.17 --, one record in four a copy of the record before it (r2 = 1 with
it).  Reported: the device milliseconds of a call, its three passes together (mg_ld_stats); the 64-bit popcounts it performs --
n_first x window x n_groups x 9, twice: the write pass forms every pair again -- per second, against the VALUs' rate for the two 32-bit
popcounts a 64-bit one takes (256 CUs x 64 lanes x 2.4 GHz / 2); and the 24 B x n_groups per record the kernel must read.
Beside each window leg the same arithmetic as a C++ loop on one host core (tools/ld_host_loop.cpp, built here with -O2 -mpopcnt
-ffp-contract=off and timed here) on the first --host-records records, scaled to all; its pairs are compared with the device's pairs of
those records bit for bit.  No ratio is promised.

    python tools/ld_bench.py [--planes 64] [--records 1000000] [--window 64] [--repeats 5] [--out profiles/ld_bench.json]
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
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from malva_amd import Context  # noqa: E402
from malva_amd.capi import LD_PAIR  # noqa: E402
from ld_model import site_words  # noqa: E402

HBM_BYTES_PER_S = 8e12
VALU_POPC64_PER_S = 256 * 64 * 2.4e9 / 2


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def host_loop(directory):
    so = os.path.join(directory, "ld_host_loop.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mpopcnt", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "ld_host_loop.cpp")], check=True)
    f = C.CDLL(so).ld_window_host
    f.argtypes = [C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]
    f.restype = C.c_uint64

    def run(sites, chrom, pos, n_first, window, max_bp, min_n, min_r2):
        G, _, n = sites.shape
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pairs, off = np.zeros(n_first * window + 1, dtype=LD_PAIR), np.zeros(n_first + 1, dtype=np.uint64)
        t0 = time.perf_counter()
        k = f(n, n_first, G, p(sites), p(chrom), p(pos), window, max_bp, min_n, min_r2, p(pairs), pairs.size, p(off))
        return pairs[:k], off, (time.perf_counter() - t0) * 1e3
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-gq", type=int, default=20)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--host-records", type=int, nargs="+", default=[100_000, 2_000], help="per entry of --groups")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ld_bench.json"))
    a = ap.parse_args()
    P, n, W = a.planes, a.records, a.window
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261020)
    out = {"workload": "ld", "planes": P, "records": n, "window": W, "repeats": a.repeats, "min_gq": a.min_gq}
    with tempfile.TemporaryDirectory() as tmp, Context(35, 43, 1 << 20) as c:
        host = host_loop(tmp)
        # ---- the pack
        af = torch.distributions.Beta(0.5, 2.0).sample((n,)).to(dev)

        def draw():
            g = (torch.rand((P, n), device=dev, generator=gen) < af[None, :]).to(torch.int32)
            stray = torch.rand((P, n), device=dev, generator=gen)
            g[stray < 0.01] = -1
            g[stray > 0.99] = 2
            return g
        g1, g2 = draw(), draw()
        gq = torch.randint(0, 120, (P, n), device=dev, generator=gen, dtype=torch.int32)
        vao = (2 * torch.arange(n + 1, device=dev)).to(torch.int32)
        words = torch.zeros((3, n), device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats + 1):                                       # (the first call creates the events: not kept)
            c.pack_site_dosage_device(n, P, False, g1.data_ptr(), g2.data_ptr(), gq.data_ptr(), vao.data_ptr(), words.data_ptr(), min_gq=a.min_gq)
            ms.append(c.ld_stats()[0])
        out["pack_ms"] = stat(ms[1:])
        k = min(n, 20_000)
        h = lambda t: t[:, :k].cpu().numpy()
        want = site_words(h(g1), h(g2), h(gq), False, np.arange(k + 1, dtype=np.uint32) * 2, a.min_gq)
        out["pack_equals_model"] = int(np.array_equal(words[:, :k].cpu().numpy().view(np.uint64), want))
        moved = 12 * P * n + 8 * n + 24 * n
        out["pack_bytes"] = moved
        out["pack_gb_per_s"] = round(moved / out["pack_ms"]["median"] / 1e6, 1)
        out["pack_expected_ms_at_half_hbm"] = round(moved / (HBM_BYTES_PER_S / 2) * 1e3, 4)
        del g1, g2, gq, words
        # ---- the window
        chrom = torch.zeros(n, device=dev, dtype=torch.int32)
        pos = (100 * torch.arange(n, device=dev) + 1).to(torch.int32)
        src = torch.arange(n, device=dev)
        copy = torch.rand(n, device=dev, generator=gen) < 0.25
        copy[0] = False
        src[copy] -= 1
        for G, host_records in zip(a.groups, a.host_records):
            half = lambda: torch.randint(0, 1 << 32, (G, n), device=dev, generator=gen, dtype=torch.int64)
            r = lambda: half() << 32 | half()                                # 64 random bits
            valid = r() | r() | r()                                          # a bit set in seven of eight cases
            u, v = r(), r() & r() | r() & r() & r()                          # u: 1/2; v: 1/4 + 3/4 * 1/8, about 0.34
            sites = torch.stack([valid & u, valid & ~u & ~v, valid & ~u & v], dim=1)[:, :, src].contiguous()
            del valid, u, v
            cap = 8 * n
            pairs = torch.zeros(3 * cap, device=dev, dtype=torch.int64)
            off = torch.zeros(n + 1, device=dev, dtype=torch.int64)
            torch.cuda.synchronize()
            ms, need = [], 0
            for _ in range(a.repeats + 1):
                rc, need = c.ld_window_device(n, n, G, sites.data_ptr(), chrom.data_ptr(), pos.data_ptr(), W, 0, 2, 0.2, pairs.data_ptr(), cap, off.data_ptr())
                assert rc == 0, "the pairs' buffer is too small: %d needed" % need
                ms.append(c.ld_stats()[1])
            med = stat(ms[1:])
            popc = 2 * n * W * G * 9
            hn = min(host_records, n)
            m = min(n, hn + W)
            h_pairs, h_off, h_ms = host(np.ascontiguousarray(sites[:, :, :m].cpu().numpy().view(np.uint64)), chrom[:m].cpu().numpy().view(np.uint32),
                                        pos[:m].cpu().numpy().view(np.uint32), hn, W, 0, 2, 0.2)
            d_off = off[:hn + 1].cpu().numpy().view(np.uint64)
            d_pairs = pairs[:3 * int(d_off[hn])].cpu().numpy().view(LD_PAIR)
            out["window_g%d" % G] = {
                "n_groups": G, "device_ms": med, "pairs": int(need), "popcounts_64": popc, "popcounts_per_s": round(popc / med["median"] * 1e3, 0),
                "share_of_valu_rate": round(popc / med["median"] * 1e3 / VALU_POPC64_PER_S, 3), "bytes_read_once": 24 * G * n,
                "read_ms_at_half_hbm": round(24 * G * n / (HBM_BYTES_PER_S / 2) * 1e3, 4),
                "host_records": hn, "host_ms": round(h_ms, 1), "host_ms_scaled_to_all_records": round(h_ms * n / max(hn, 1), 0),
                "host_equals_device_bits": int(np.array_equal(h_off, d_off) and h_pairs.tobytes() == d_pairs.tobytes())}
            del sites, pairs, off
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
