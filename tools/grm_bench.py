"""The kernels behind `call --cohort --grm` on one MI355X, through the C ABI's device forms (the words are made on the device with torch, so
no leg pays a copy).

A leg is mg_grm_begin, --records records in steps of --chunk through mg_grm_step_device, and one mg_grm_read, at 64, 1,024 and 4,096
samples: a cell contributes in seven of eight cases, with dosage 2 in a quarter and dosage 1 in three eighths of those, so every record
enters.  Reported: the device milliseconds of all steps (the sums of mg_grm_stats[0], weights + expansion, and of mg_grm_stats[1], the Gram
kernel), the median of --repeats legs with their spread, and the read.
EXPECTATIONS, written before any run.  Expansion: it writes 3 B per padded sample and record and reads 24 B per group and record; it should
reach half the HBM rate of 8 TB/s for those bytes.  Gram: five i8 multiply-adds per pair a <= b and record; v_mfma_i32_16x16x64_i8 takes the
16 cycles of the bf16 16x16x32 form, 1,024 multiply-adds per clock and SIMD, 2.5e15 per second on 1,024 SIMDs at 2.4 GHz; a quarter or more
of that rate would meet it.  At 64 samples the device is underfilled however the records are split: known and accepted.
Beside each leg the definition as a C++ loop on one host core (tools/grm_host_loop.cpp, built here with -O2 and timed here) over the first
--host-records records and the pairs of the first --host-rows rows, scaled to all; its sums are compared with the device's sums of those
pairs after those records, value by value.  No ratio is promised.

    python tools/grm_bench.py [--records 1000000] [--chunk 65536] [--repeats 5] [--out profiles/grm_bench.json]
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
from malva_amd import Context  # noqa: E402

HBM_BYTES_PER_S = 8e12
I8_MAC_PER_S = 1024 * 1024 * 2.4e9      # multiply-adds per clock and SIMD x SIMDs x clock
PRODUCTS = 5


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def host_loop(directory):
    so = os.path.join(directory, "grm_host_loop.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "grm_host_loop.cpp")], check=True)
    f = C.CDLL(so).grm_step_host
    f.argtypes = [C.c_size_t, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    f.restype = C.c_uint64

    def run(sites, n_samples, maf_ppm, min_n, rows):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        k = n_samples * (n_samples + 1) // 2
        S, N = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.uint64)
        t0 = time.perf_counter()
        entered = f(sites.shape[2], n_samples, p(sites), 0, maf_ppm, min_n, rows, p(S), p(N))
        return S, N, int(entered), (time.perf_counter() - t0) * 1e3
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--chunk", type=int, default=65_536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--host-records", type=int, default=20_000)
    ap.add_argument("--host-rows", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grm_bench.json"))
    a = ap.parse_args()
    n = a.records
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261020)
    maf_ppm, min_n = 10000, 2
    out = {"workload": "grm", "records": n, "chunk": a.chunk, "repeats": a.repeats, "maf_ppm": maf_ppm, "min_n": min_n}

    def random_bits(G):
        half = lambda: torch.randint(0, 1 << 32, (G, n), device=dev, generator=gen, dtype=torch.int64)
        return half() << 32 | half()

    def make_sites(G):
        valid = random_bits(G) | random_bits(G) | random_bits(G)                # seven of eight
        two, one = random_bits(G) & random_bits(G), random_bits(G)              # 1/4, 1/2
        return torch.stack([valid & ~two & ~one, valid & ~two & one, valid & two], dim=1).contiguous()

    with tempfile.TemporaryDirectory() as tmp, Context(35, 43, 1 << 20) as c:
        host = host_loop(tmp)
        for S in a.samples:
            G = (S + 63) // 64
            rows = (S + 31) // 32 * 32
            sites = make_sites(G)
            chunks = [(c0, min(n, c0 + a.chunk)) for c0 in range(0, n, a.chunk)]
            parts = [sites[:, :, c0:c1].contiguous() for c0, c1 in chunks]      # (a chunk's words are contiguous, as the pass hands them over)
            hn = min(a.host_records, n)
            head = sites[:, :, :hn].contiguous()
            torch.cuda.synchronize()
            c.grm_begin(S, False, maf_ppm, min_n)                                # the host's records alone, for the comparison
            c.grm_step_device(hn, G, head.data_ptr())
            d_S, d_N, _, d_entered = c.grm_read(S)
            legs_expand, legs_gram, reads, entered = [], [], [], 0
            for rep in range(a.repeats + 1):                                    # (the first leg creates the events and the scratch: not kept)
                c.grm_begin(S, False, maf_ppm, min_n)
                ms_e = ms_g = 0.0
                for i, (c0, c1) in enumerate(chunks):
                    c.grm_step_device(c1 - c0, G, parts[i].data_ptr())
                    ms = c.grm_stats()
                    ms_e, ms_g = ms_e + ms[0], ms_g + ms[1]
                _, _, seen, entered = c.grm_read(S)
                assert seen == n
                legs_expand.append(ms_e), legs_gram.append(ms_g), reads.append(c.grm_stats()[2])
            c.grm_end()
            e, g = stat(legs_expand[1:]), stat(legs_gram[1:])
            pairs = S * (S + 1) // 2
            macs = PRODUCTS * pairs * n
            moved = (3 * rows + 24 * G + 16) * n
            hr = min(a.host_rows, S)
            h_S, h_N, h_entered, h_ms = host(np.ascontiguousarray(head.cpu().numpy().view(np.uint64)), S, maf_ppm, min_n, hr)
            h_pairs = sum(S - r for r in range(hr))
            same = h_entered == d_entered and np.array_equal(h_S[:h_pairs], d_S[:h_pairs]) and np.array_equal(h_N[:h_pairs], d_N[:h_pairs])
            out["grm_s%d" % S] = {
                "n_samples": S, "pairs": pairs, "steps": len(chunks), "records_entered": int(entered),
                "expand_ms": e, "expand_bytes": moved, "expand_gb_per_s": round(moved / e["median"] / 1e6, 1), "expand_expected_ms_at_half_hbm": round(moved / (HBM_BYTES_PER_S / 2) * 1e3, 3),
                "expand_share_of_hbm_rate": round(moved / e["median"] * 1e3 / HBM_BYTES_PER_S, 3), "expand_expectation_met": int(moved / e["median"] * 1e3 >= HBM_BYTES_PER_S / 2),
                "gram_ms": g, "gram_macs": macs, "gram_macs_per_s": round(macs / g["median"] * 1e3, 0), "gram_ms_at_i8_rate": round(macs / I8_MAC_PER_S * 1e3, 3),
                "gram_share_of_i8_rate": round(macs / g["median"] * 1e3 / I8_MAC_PER_S, 4), "gram_expectation_met": int(macs / g["median"] * 1e3 >= I8_MAC_PER_S / 4),
                "read_ms": stat(reads[1:]),
                "host_records": hn, "host_rows": hr, "host_pairs": h_pairs, "host_ms": round(h_ms, 1), "host_ms_scaled_to_all": round(h_ms * (pairs / h_pairs) * (n / hn), 0),
                "host_equals_device": int(same)}
            del sites, parts, head
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
