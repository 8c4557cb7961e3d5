"""A cohort of S samples against one resident index on one MI355X: the per-sample device time of the single-sample entry points
(reset -> scan -> mg_cover_blocks_device -> mg_genotype_device, sample after sample) against cohort mode (S planes scanned, one
mg_cover_blocks_cohort_device over all of them, mg_genotype_device per plane), on two recipes:

    c3   1e6 isolated SNPs (synth.snp_panel as a FlatPanel), tables of 1e7 rows
    c4   the clustered SNP panel at the size tests/test_gpu_resident.py uses (1.2e6 records on one sequence), tables of 3e6 rows

Device milliseconds from HIP events on the context's stream, one warm-up, the median of --repeats with their spread.  Every sample
scans the same rows with its own counts (the scan's time does not depend on the counts).  Writes one JSON object to
profiles/cohort_bench.json and prints it.

    python tools/cohort_bench.py [--samples 16] [--repeats 5] [--recipes c3,c4] [--baseline-only] [--cli [--parent-bin PATH]] [--out profiles/cohort_bench.json]

--baseline-only touches nothing of cohort mode: it runs on a build that does not have it.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from malva_amd import BF_ALT, BF_CTX, Context, synth  # noqa: E402
from malva_amd.resident import ResidentPanel  # noqa: E402

K, REF_K = 35, 43


def recipe(name):
    if name == "c3":
        return synth.flat_from_snp_panel(synth.snp_panel(1_000_000, seed=20261016)), 4 << 33, 10_000_000, 200_000
    if name == "c4":
        return synth.clustered_snp_panel(1_200_000, seed=41, n_contigs=1), 1 << 30, 3_000_000, 20_000
    raise SystemExit("unknown recipe %s" % name)


class Timer:
    def __init__(self, stream):
        self.stream, self.marks = stream, []

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record(self.stream)
        self.marks.append((name, e))

    def spans(self):
        torch.cuda.synchronize()
        out = {}
        for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return out


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def run_recipe(name, S, repeats, baseline_only):
    panel, bits, n_rows, plant = recipe(name)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = Context(K, REF_K, bits, device=0)
    ctx.set_stream(stream.cuda_stream)
    ctx.reference_upload(panel.genome)
    rp = ResidentPanel(panel, 0, haploid=False)
    rp.index(ctx)
    ctx.bf_finalize(BF_ALT)
    for b, l in zip(panel.contig_base, panel.contig_len):
        ctx.ref_scan_resident(int(b), int(l))
    ctx.bf_finalize(BF_CTX)
    tab = synth.device_table_flat(panel, n_rows, K, REF_K, 7, dev, plant_records=plant)
    cnts = [((tab["d_cnt"].to(torch.int64) * (2 * s + 1) + 7 * s) % 200 + 1).to(torch.int32) for s in range(S)]
    torch.cuda.synchronize()
    n_bf, n_map = ctx.counters_size()
    out = {"records": int(panel.n), "table_rows": n_rows, "samples": S, "bf_counters": n_bf, "map_counters": n_map}

    def scan(s):
        ctx.kmc_scan_device(tab["d_hi"].data_ptr(), tab["d_lo"].data_ptr(), cnts[s].data_ptr(), n_rows)

    def baseline(record_counters):
        ctx.set_option("use_record_counters", record_counters)
        per = {"scan": [], "cover": [], "genotype": [], "total": [], "tier1": [], "tiers23": []}
        covs = []
        for rep in range(repeats + 1):
            t = Timer(stream)
            t.mark("start")
            for s in range(S):
                ctx.counters_reset()
                scan(s)
                t.mark("scan")
                rp.cut(ctx)
                rp.cover(ctx)
                t.mark("cover")
                rp.genotype(ctx, probs=False)
                t.mark("genotype")
                if rep == 0:
                    covs.append(rp.results()["cov"].copy())
                elif s == S - 1:
                    # the same bracket as mg_cohort_stats' two figures: mg_blocks_stats' tier 1 (set-up + the lone kernels) and tiers 2 + 3
                    # (waits for the device: taken once per repeat, after the last sample, so that the spans above stay back to back)
                    bs = ctx.blocks_stats()
                    per["tier1"].append(bs[0])
                    per["tiers23"].append(bs[1] + bs[2])
            sp = t.spans()
            if rep:  # (the first pass warms up)
                for key in ("scan", "cover", "genotype"):  # ("cover" = the cut + mg_cover_blocks_device: tier 1, tiers 2-3 and the final pass)
                    per[key].append(sp[key] / S)
                per["total"].append(sum(sp.values()) / S)
        return {key: stat(v) for key, v in per.items()}, covs

    out["baseline_ms_per_sample"], covs = baseline(1)                # as a `call` runs by default
    out["baseline_vectors_only_ms_per_sample"], _ = baseline(0)      # the counters in the vectors alone, as cohort mode keeps them
    ctx.set_option("use_record_counters", 1)
    if not baseline_only:
        from malva_amd.resident import ResidentCohort
        per = {"scan": [], "cut": [], "tier1": [], "tiers23": [], "genotype": [], "total": []}
        equal = True
        for rep in range(repeats + 1):
            co = ResidentCohort(rp, ctx, S)
            t = Timer(stream)
            t.mark("start")
            for s in range(S):
                co.select(s)
                scan(s)
            t.mark("scan")
            rp.cut(ctx)
            t.mark("cut")
            co.cover()
            t.mark("cover")
            co.genotype(probs=False)
            t.mark("genotype")
            sp = t.spans()
            t1, t23 = ctx.cohort_stats()
            if rep == 0:
                equal = all(np.array_equal(co.results(s)["cov"], covs[s]) for s in range(S))
            else:
                per["scan"].append(sp["scan"] / S)
                per["cut"].append(sp["cut"] / S)
                per["tier1"].append(t1 / S)
                per["tiers23"].append(t23 / S)
                per["genotype"].append(sp["genotype"] / S)
                per["total"].append(sum(sp.values()) / S)
            co.close()
        out["cohort_ms_per_sample"] = {key: stat(v) for key, v in per.items()}
        out["cohort_equals_baseline"] = bool(equal)
    ctx.close()
    return out


def run_cli(S, snps, rows, parent_bin):
    """wall time of `malva-geno call --cohort` on S samples against S single calls (this build's binary and, if given, another
    build's: the parent commit's), same files: a panel of `snps` isolated SNPs, one text dump of `rows` k-mers that every sample
    names (the work per sample is the same; only the names differ)"""
    import subprocess
    import tempfile
    import time
    binp = os.path.join(ROOT, "bin", "malva-geno")
    panel = synth.flat_from_snp_panel(synth.snp_panel(snps, seed=20261016))
    out = {"snps": snps, "table_rows": rows, "samples": S}
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, "c3")
        synth.write_vcf_fasta(panel, prefix)
        hi, lo, _ = synth.flat_kmer_table(panel, rows, K, REF_K, seed=7, max_records=min(snps, 200_000))
        text = synth.unpack_ascii(hi, lo, REF_K, stride=REF_K + 4)          # KMER<tab>NN<newline>, two-digit counts
        cnt = 10 + (np.arange(len(hi)) * 7) % 50
        text[:, REF_K] = 9
        text[:, REF_K + 1] = 48 + cnt // 10
        text[:, REF_K + 2] = 48 + cnt % 10
        text[:, REF_K + 3] = 10
        with open(os.path.join(td, "sample.txt"), "wb") as fh:
            fh.write(text.tobytes())
        with open(os.path.join(td, "cohort.tsv"), "w") as fh:
            fh.write("".join("s%02d\tsample\n" % i for i in range(S)))
        common = ["-k", str(K), "-r", str(REF_K), "-b", "4", prefix + ".fa", prefix + ".vcf"]
        subprocess.run([binp, "index"] + common + [os.path.join(td, "sample")], check=True, capture_output=True, timeout=600)

        def singles(b):
            t0 = time.perf_counter()
            for _ in range(S):
                r = subprocess.run([b, "call"] + common + [os.path.join(td, "sample")], capture_output=True, timeout=600)
                assert r.returncode == 0, r.stderr[-500:]
            return round(time.perf_counter() - t0, 2), r.stdout
        singles(binp)                                                        # (warms the page cache)
        out["single_calls_wall_s"], want = singles(binp)
        if parent_bin:
            out["single_calls_other_build_wall_s"], other = singles(parent_bin)
            out["other_build_same_bytes"] = other == want
        t0 = time.perf_counter()
        r = subprocess.run([binp, "call", "--cohort", "-o", os.path.join(td, "out")] + common[:-2] + [prefix + ".fa", prefix + ".vcf", os.path.join(td, "cohort.tsv")],
                           capture_output=True, timeout=900, env=dict(os.environ, MALVA_GENO_TIMERS="1"))
        out["cohort_wall_s"] = round(time.perf_counter() - t0, 2)
        assert r.returncode == 0, r.stderr[-500:]
        out["cohort_timers"] = [l.split("]", 1)[1].strip() for l in r.stderr.decode().split("\n") if "timer]" in l and "cohort" in l]
        out["cohort_same_bytes"] = all(open(os.path.join(td, "out", "s%02d.vcf" % i), "rb").read() == want for i in range(S))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--recipes", default="c3,c4")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--cli", action="store_true", help="also: wall time of `call --cohort` against S single calls")
    ap.add_argument("--cli-snps", type=int, default=1_000_000)
    ap.add_argument("--cli-rows", type=int, default=2_000_000)
    ap.add_argument("--parent-bin", default=None, help="--cli: a malva-geno of another build (the parent commit's) to time the single calls with as well")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cohort_bench.json"))
    a = ap.parse_args()
    out = {"workload": "cohort", "k": K, "ref_k": REF_K, "baseline_only": a.baseline_only, "device": torch.cuda.get_device_name(0)}
    for name in a.recipes.split(","):
        out[name] = run_recipe(name, a.samples, a.repeats, a.baseline_only)
    if a.cli:
        out["cli"] = run_cli(a.samples, a.cli_snps, a.cli_rows, a.parent_bin)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
