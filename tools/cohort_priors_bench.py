"""mg_genotype_cohort_device on one MI355X against what the batch costs today: n_planes calls of mg_genotype_device on the same arrays.

Workload: 64 planes x 1e6 biallelic records, diploid, every array resident on the device.  A record's cohort frequency is drawn from
0.02..0.6 and is not the panel's AF (0.003); a plane's genotype is drawn from it, its reads at a depth of 5..40 split by the
genotype; one cell in twenty has no coverage.

Timed on the context's stream with events (a warm-up run of every leg first, then --repeats runs each, interleaved; the median and the
spread are kept):
    plain      the n_planes calls of mg_genotype_device, plane by plane -- the existing entry, timed in the same run
    cohort_T   one mg_genotype_cohort_device at T = 0, 1 and 5 iterations (weight 1); its own timer (mg_cohort_prior_stats) beside it
    ratio_T    cohort_T / plain, from the medians
The calls of the T = 0 leg are compared with the plain leg's (same arrays): cohort_t0_equals_plain.

    python tools/cohort_priors_bench.py [--planes 64] [--records 1000000] [--repeats 7] [--out profiles/cohort_priors_bench.json]

--leg estimate_wide: mg_estimate_priors_device beyond one wave of planes.  Workload: 256 planes x 1e6 biallelic records made the same
way (2 GB of coverages).  Timed the same way, in one run:
    estimate_T   one mg_estimate_priors_device over all planes at T = 0, 1 and 5; its own timer (mg_estimate_priors_stats) beside it
    cohort4_T    planes / 64 calls of mg_genotype_cohort_device at 64 planes each on the same arrays (the estimate of 64 planes AND their
                 calls: what a cohort of that size costs as separate groups of 64, without a cohort-wide estimate)
estimate64_equals_cohort: the estimate of the first 64 planes against mg_genotype_cohort's freq_out and n_informative on them, T = 5.

    python tools/cohort_priors_bench.py --leg estimate_wide [--planes 256] [--records 1000000] [--repeats 7] [--out profiles/cohort_priors_wide_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from malva_amd.capi import Context  # noqa: E402

E, MAX_COV = 0.001, 200


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def workload(P, n, dev):
    """-> (cov [P][2n] int32 holding the u32 values, freq [2n], var_allele_off [n + 1]) on the device"""
    g = torch.Generator(device=dev)
    g.manual_seed(20261018)
    q = 0.02 + 0.58 * torch.rand(n, device=dev, generator=g)
    copies = (torch.rand(P, n, device=dev, generator=g) < q).to(torch.int32) + (torch.rand(P, n, device=dev, generator=g) < q).to(torch.int32)
    depth = torch.randint(5, 41, (P, n), device=dev, generator=g, dtype=torch.int32)
    depth = torch.where(torch.rand(P, n, device=dev, generator=g) < 0.05, torch.zeros_like(depth), depth)
    alt = depth * copies // 2
    cov = torch.stack((depth - alt, alt), dim=2).reshape(P, 2 * n).contiguous()      # [P][slots] int32 holding the u32 values
    freq = torch.tensor([0.997, 0.003], dtype=torch.float32, device=dev).repeat(n).contiguous()
    vao = (2 * torch.arange(n + 1, device=dev, dtype=torch.int64)).to(torch.int32).contiguous()
    return cov, freq, vao


def timed_on(stream):
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)
    return timed


def write_out(path, out):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def estimate_wide(a):
    P, n = a.planes or 256, a.records
    assert P % 64 == 0 and P > 64, "--leg estimate_wide takes a multiple of 64 planes above 64"
    dev = torch.device("cuda:0")
    cov, freq, vao = workload(P, n, dev)
    new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    freq_out, n_inf = new(2 * n, torch.float32), new(n, torch.int32)
    f64, n64 = new(2 * n, torch.float32), new(n, torch.int32)
    coh = [new((64, n), torch.int32) for _ in range(3)] + [new((64, n), torch.uint8)]
    stream = torch.cuda.Stream()
    out = {"workload": "cohort-priors-wide", "planes": P, "records": n, "alleles": 2, "haploid": 0, "max_cov": MAX_COV, "weight": 1.0, "repeats": a.repeats,
           "coverage_bytes": 4 * P * 2 * n}
    with torch.cuda.stream(stream), Context(35, 43, 1 << 20) as ctx:
        ctx.set_stream(stream.cuda_stream)
        timed = timed_on(stream)

        def run_estimate(T, planes=P, fo=freq_out, ni=n_inf):
            ctx.estimate_priors_device(n, planes, cov.data_ptr(), freq.data_ptr(), vao.data_ptr(), E, MAX_COV, False, T, 1.0, fo.data_ptr(), ni.data_ptr())

        def run_cohort4(T):
            for j in range(P // 64):
                ctx.genotype_cohort_device(n, 64, cov[64 * j].data_ptr(), freq.data_ptr(), vao.data_ptr(), E, MAX_COV, False, T, 1.0, f64.data_ptr(), n64.data_ptr(),
                                           coh[0].data_ptr(), coh[1].data_ptr(), coh[2].data_ptr(), coh[3].data_ptr())

        legs = {}
        for T in (0, 1, 5):
            legs["estimate_%d" % T] = lambda T=T: run_estimate(T)
            legs["cohort4_%d" % T] = lambda T=T: run_cohort4(T)
        for fn in legs.values():                                                   # warm-up: tables, code objects, clocks
            timed(fn)
        ctx.genotype_cohort_device(n, 64, cov.data_ptr(), freq.data_ptr(), vao.data_ptr(), E, MAX_COV, False, 5, 1.0, f64.data_ptr(), n64.data_ptr(),
                                   coh[0].data_ptr(), coh[1].data_ptr(), coh[2].data_ptr(), coh[3].data_ptr())
        run_estimate(5, 64)
        stream.synchronize()
        out["estimate64_equals_cohort"] = int(torch.equal(freq_out.view(torch.int32), f64.view(torch.int32)) and torch.equal(n_inf, n64))
        ms = {leg: [] for leg in legs}
        own = {leg: [] for leg in legs if leg.startswith("estimate")}
        for _ in range(a.repeats):
            for leg, fn in legs.items():
                ms[leg].append(timed(fn))
                if leg in own:
                    own[leg].append(ctx.estimate_priors_stats())
        run_estimate(5)
        stream.synchronize()
        out["t5_records_moved"] = round((freq_out.view(n, 2)[:, 1] != 0.003).float().mean().item(), 4)
        out["t5_n_informative_mean"] = round(n_inf.float().mean().item(), 2)
    for leg in legs:
        out[leg + "_ms"] = stat(ms[leg])
    for leg in own:
        out[leg + "_own_timer_ms"] = stat(own[leg])
        out["ratio_" + leg[9:]] = round(float(np.median(ms[leg]) / np.median(ms["cohort4_" + leg[9:]])), 3)
    write_out(a.out or os.path.join(ROOT, "profiles", "cohort_priors_wide_bench.json"), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("cohort", "estimate_wide"), default="cohort")
    ap.add_argument("--planes", type=int, default=0)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.leg == "estimate_wide":
        return estimate_wide(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "cohort_priors_bench.json")
    P, n = a.planes or 64, a.records
    dev = torch.device("cuda:0")
    cov, freq, vao = workload(P, n, dev)
    new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    freq_out, n_inf = new(2 * n, torch.float32), new(n, torch.int32)
    plain = [new((P, n), torch.int32) for _ in range(3)] + [new((P, n), torch.uint8)]
    coh = [new((P, n), torch.int32) for _ in range(3)] + [new((P, n), torch.uint8)]
    stream = torch.cuda.Stream()
    out = {"workload": "cohort-priors", "planes": P, "records": n, "alleles": 2, "haploid": 0, "max_cov": MAX_COV, "weight": 1.0, "repeats": a.repeats}
    with torch.cuda.stream(stream), Context(35, 43, 1 << 20) as ctx:
        ctx.set_stream(stream.cuda_stream)
        timed = timed_on(stream)

        def run_plain():
            for p in range(P):
                ctx.genotype_device(cov[p].data_ptr(), freq.data_ptr(), vao.data_ptr(), n, E, MAX_COV, False, plain[0][p].data_ptr(), plain[1][p].data_ptr(),
                                    plain[2][p].data_ptr(), plain[3][p].data_ptr())

        def run_cohort(T):
            ctx.genotype_cohort_device(n, P, cov.data_ptr(), freq.data_ptr(), vao.data_ptr(), E, MAX_COV, False, T, 1.0, freq_out.data_ptr(), n_inf.data_ptr(),
                                       coh[0].data_ptr(), coh[1].data_ptr(), coh[2].data_ptr(), coh[3].data_ptr())

        legs = {"plain": run_plain, "cohort_0": lambda: run_cohort(0), "cohort_1": lambda: run_cohort(1), "cohort_5": lambda: run_cohort(5)}
        for fn in legs.values():                                                   # warm-up: tables, code objects, clocks
            timed(fn)
        run_plain()
        run_cohort(0)
        stream.synchronize()
        out["cohort_t0_equals_plain"] = int(all(torch.equal(x, y) for x, y in zip(plain, coh)))
        ms = {leg: [] for leg in legs}
        own = {leg: [] for leg in legs if leg != "plain"}
        for _ in range(a.repeats):
            for leg, fn in legs.items():
                ms[leg].append(timed(fn))
                if leg in own:
                    own[leg].append(ctx.cohort_prior_stats())
        run_cohort(5)
        stream.synchronize()
        moved = (freq_out.view(n, 2)[:, 1] != 0.003).float().mean().item()
        out["t5_records_moved"] = round(moved, 4)
        out["t5_cells_called_otherwise"] = round(((coh[0] != plain[0]) | (coh[1] != plain[1])).float().mean().item(), 5)
    for leg in legs:
        out[leg + "_ms"] = stat(ms[leg])
    for leg in own:
        out[leg + "_own_timer_ms"] = stat(own[leg])
        out["ratio_" + leg[7:]] = round(float(np.median(ms[leg]) / np.median(ms["plain"])), 3)
    write_out(a.out, out)


if __name__ == "__main__":
    main()
