"""The kernels behind `call --cohort --ibd` on one MI355X, through the C ABI's device forms (the tables are made on the device with torch, so
no leg pays a copy).

Transpose legs: mg_sites_to_planes on --records records for n_groups 1 and 256, random words.  Reported: the device milliseconds of a call
(mg_ibd_stats[0]: the kernel alone), the median of --repeats calls with their spread; the bytes it must move -- 24 B read and 24 B written per
record and group -- and the time those take at half the HBM rate of 8 TB/s.  EXPECTATION, written before any run: the kernel is bound by memory
and should reach about half the HBM rate.  A slice of the planes is compared with tests/ibd_model.py.
Step legs: a walk over --records records in chunks of --chunk through mg_ibd_begin / mg_ibd_step at 64, 1,024 and 4,096 samples: a cell
contributes in seven of eight cases, dosage 2 in about 0.2 % and dosage 1 in 12.5 % of those, so a pair's record is DISC in about 0.2 % of the cases and
one word in ten takes the slow path; three contigs.  min_records is --min-records (3,000: about one run in six thousand is that long, so the table stays a few million segments at
4,096 samples and the host's pairs still have some), min_bp 0.  Reported: the device milliseconds of the walk (the sum of mg_ibd_stats[1] over its steps: transpose, start words, length
pass, scan, write pass), the median of --repeats walks; pairs x words, twice (the write pass walks again); and the integer operations per second
that makes at 15 per pair and word against the VALUs' 32-bit rate (256 CUs x 64 lanes x 2.4 GHz, the figure tools/ld_bench.py uses).
EXPECTATION, written before any run: the walk is bound by the VALUs, about 15 integer operations and two LDS reads per pair and word on the fast
path; a share of the VALU rate of a quarter or more would meet it.  At 64 samples the device is underfilled (eight workgroups): known and accepted.
Beside each step leg the definition as a C++ loop on one host core (tools/ibd_host_loop.cpp, built here with -O2 and timed here) over the
pairs of the first --host-samples samples, scaled to all pairs; its segments are compared with the device's segments of those pairs field by
field.  No ratio is promised.

    python tools/ibd_bench.py [--records 1000000] [--chunk 65536] [--repeats 5] [--out profiles/ibd_bench.json]
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
from malva_amd.capi import IBD_SEG  # noqa: E402
from ibd_model import planes_from_words  # noqa: E402

HBM_BYTES_PER_S = 8e12
VALU_OPS_PER_S = 256 * 64 * 2.4e9
OPS_PER_PAIR_WORD = 15


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def host_loop(directory):
    so = os.path.join(directory, "ibd_host_loop.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "ibd_host_loop.cpp")], check=True)
    f = C.CDLL(so).ibd_walk_host
    f.argtypes = [C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_size_t]
    f.restype = C.c_uint64

    def run(sites, chrom, pos, n_samples, min_records, min_bp, cap):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        segs = np.zeros(cap, dtype=IBD_SEG)
        t0 = time.perf_counter()
        k = f(sites.shape[2], n_samples, p(sites), p(chrom), p(pos), min_records, min_bp, p(segs), cap)
        assert k <= cap
        return segs[:k], (time.perf_counter() - t0) * 1e3
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--chunk", type=int, default=65_536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-records", type=int, default=3_000)
    ap.add_argument("--transpose-groups", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--host-samples", type=int, default=8)
    ap.add_argument("--segs-cap", type=int, default=1 << 24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ibd_bench.json"))
    a = ap.parse_args()
    n = a.records
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261020)
    out = {"workload": "ibd", "records": n, "chunk": a.chunk, "repeats": a.repeats, "min_records": a.min_records, "min_bp": 0}

    def random_bits(G):
        half = lambda: torch.randint(0, 1 << 32, (G, n), device=dev, generator=gen, dtype=torch.int64)
        return half() << 32 | half()

    def and_of(G, k):
        x = random_bits(G)
        for _ in range(k - 1):
            x &= random_bits(G)
        return x

    def make_sites(G):
        valid = random_bits(G) | random_bits(G) | random_bits(G)                # seven of eight
        two, one = and_of(G, 9), and_of(G, 3)                                   # 2^-9, 2^-3
        return torch.stack([valid & ~two & ~one, valid & ~two & one, valid & two], dim=1).contiguous()

    with tempfile.TemporaryDirectory() as tmp, Context(35, 43, 1 << 20) as c:
        host = host_loop(tmp)
        W = (n + 63) // 64
        # ---- the transpose
        for G in a.transpose_groups:
            sites = torch.stack([random_bits(G) for _ in range(3)], dim=1).contiguous()
            planes = torch.zeros((64 * G, 3, W), device=dev, dtype=torch.int64)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.repeats + 1):                                      # (the first call creates the events: not kept)
                c.sites_to_planes_device(n, G, sites.data_ptr(), planes.data_ptr())
                ms.append(c.ibd_stats()[0])
            med = stat(ms[1:])
            k = min(n, 6_400)
            want = planes_from_words(sites[:1, :, :k].cpu().numpy().view(np.uint64))
            got = planes[:64, :, :k // 64].cpu().numpy().view(np.uint64)
            moved = 48 * G * n
            out["transpose_g%d" % G] = {"n_groups": G, "device_ms": med, "bytes": moved, "gb_per_s": round(moved / med["median"] / 1e6, 1),
                                        "expected_ms_at_half_hbm": round(moved / (HBM_BYTES_PER_S / 2) * 1e3, 4),
                                        "share_of_hbm_rate": round(moved / med["median"] * 1e3 / HBM_BYTES_PER_S, 3),
                                        "equals_model": int(np.array_equal(got, want[:, :, :k // 64]))}
            del sites, planes
        # ---- the steps
        chrom = (torch.arange(n, device=dev) * 3 // n).to(torch.int32)
        pos = (100 * (torch.arange(n, device=dev) % ((n + 2) // 3)) + 1).to(torch.int32)
        segs = torch.zeros(4 * a.segs_cap, device=dev, dtype=torch.int64)
        for S in a.samples:
            G = (S + 63) // 64
            sites = make_sites(G)
            if S % 64:
                sites[G - 1] &= (1 << (S % 64)) - 1
            chunks = [(c0, min(n, c0 + a.chunk)) for c0 in range(0, n, a.chunk)]
            parts = [sites[:, :, c0:c1].contiguous() for c0, c1 in chunks]      # (a chunk's words are contiguous, as the pass hands them over)
            torch.cuda.synchronize()
            walks, total, kept = [], 0, None
            for rep in range(a.repeats + 1):
                c.ibd_begin(S, a.min_records, 0)
                ms, total, mine = 0.0, 0, []
                for i, (c0, c1) in enumerate(chunks):
                    rc, need = c.ibd_step_device(c1 - c0, G, parts[i].data_ptr(), chrom[c0:c1].data_ptr(), pos[c0:c1].data_ptr(), i == len(chunks) - 1, segs.data_ptr(), a.segs_cap)
                    assert rc == 0, "the segments' buffer is too small: %d needed" % need
                    ms += c.ibd_stats()[1]
                    total += need
                    if rep == 0 and need:                                        # the first walk's segments of the host's pairs, for the comparison
                        s = segs[:4 * need].cpu().numpy().view(IBD_SEG)
                        mine.append(s[s["b"] < a.host_samples].copy())
                if rep == 0:
                    kept = np.concatenate(mine) if mine else np.zeros(0, dtype=IBD_SEG)
                walks.append(ms)
                c.ibd_end()
            med = stat(walks[1:])
            pairs = S * (S - 1) // 2
            pair_words = 2 * pairs * W
            hs = min(a.host_samples, S)
            h_segs, h_ms = host(np.ascontiguousarray(sites[:1].cpu().numpy().view(np.uint64)), chrom.cpu().numpy().view(np.uint32), pos.cpu().numpy().view(np.uint32), hs,
                                a.min_records, 0, 1 << 20)
            key = kept["a"].astype(np.int64) << 32 | kept["b"].astype(np.int64)
            kept = kept[np.argsort(key, kind="stable")]
            ops = pair_words * OPS_PER_PAIR_WORD
            out["step_s%d" % S] = {
                "n_samples": S, "pairs": pairs, "steps": len(chunks), "device_ms": med, "segments": int(total), "pair_words_both_passes": pair_words,
                "pair_words_per_s": round(pair_words / med["median"] * 1e3, 0), "ops_per_s_at_15_per_pair_word": round(ops / med["median"] * 1e3, 0),
                "share_of_valu_rate": round(ops / med["median"] * 1e3 / VALU_OPS_PER_S, 3), "expected_ms_at_valu_rate": round(ops / VALU_OPS_PER_S * 1e3, 3),
                "host_samples": hs, "host_pairs": hs * (hs - 1) // 2, "host_ms": round(h_ms, 1), "host_ms_scaled_to_all_pairs": round(h_ms * pairs / max(hs * (hs - 1) // 2, 1), 0),
                "host_segments": int(len(h_segs)), "host_equals_device": int(h_segs.tobytes() == kept.tobytes())}
            del sites, parts
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
