"""`call --cohort --merged` against `call --cohort -o` on one MI355X, on the input of tools/cohort_bench.py --cli: a panel of 1e6
isolated SNPs, 16 samples that all name one text dump of 2e6 k-mers.

Timed, each the median of --repeats runs with their spread:
    per_sample   `--cohort -o OUTDIR`         wall time and the `cohort: panel pass` timer (MALVA_GENO_TIMERS=1)
    merged       `--cohort --merged PATH`     the same two, and the device milliseconds per mg_format_calls (mg_format_stats)
    merged_tags  the same with `--min-gq Q --site-tags` (Q: --min-gq, default 20): the same, and the device milliseconds per
                 mg_site_counts and per mg_format_site_info (mg_site_stats) beside them
    merged_bcf   `--cohort --merged PATH --merged-format bcf`, merged_ubcf the same with ubcf: the same two, the bytes written, and
                 the device milliseconds per mg_encode_calls_bcf (mg_bcf_stats) -- on the batches the merged leg formats as text
    merged_gp    `--cohort --merged PATH --gp`, merged_gp_bcf the same with `--merged-format bcf`: the same two, the bytes written and
                 the device milliseconds per mg_format_calls / mg_encode_calls_bcf with MG_CELLS_GP in their mg_cells (mg_format_stats / mg_bcf_stats)
    merged_pl    `--cohort --merged PATH --pl`, merged_pl_bcf the same with `--merged-format bcf`: the same two, the bytes written, the
                 device milliseconds per mg_format_calls / mg_encode_calls_bcf with MG_CELLS_PL and per mg_phred_likelihoods (mg_pl_stats); with
                 --parent-bin the parent commit's own `merged` / `merged_bcf` legs run beside them on the same input (parent_merged,
                 parent_merged_bcf): what the two legs are compared with
    parent       `--cohort -o OUTDIR` with --parent-bin, the malva-geno of the parent commit: the yardstick; parent_verdict then holds,
                 for the wall time and the panel pass, both medians, the parent's own spread (max - min) and whether per_sample's median
                 lies within it
The runs alternate (parent, per_sample, merged, parent, ...), so that whatever else the host is doing falls on all three alike.
merged_equals_paste: the merged file is the column paste of the per-sample files.

    python tools/merged_bench.py [--samples 16] [--snps 1000000] [--rows 2000000] [--repeats 3] [--parent-bin PATH] [--out profiles/cohort_merged_bench.json]

--leg pl_device: no command line; mg_phred_likelihoods_device alone, one call over 64 planes x 1e6 biallelic diploid records -- the arrays of
tools/cohort_priors_bench.py -- against the 64 calls of mg_genotype_device on the same arrays in the same run (events on the context's
stream, a warm-up, then --repeats interleaved runs, medians and spread).  The result goes under "pl_device" of the same file, beside what is there.

    python tools/merged_bench.py --leg pl_device [--planes 64] [--records 1000000] [--repeats 7]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from malva_amd import synth  # noqa: E402

K, REF_K = 35, 43
BIN = os.path.join(ROOT, "bin", "malva-geno")


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def timer(stderr, label):
    m = re.search(r"timer\] %s\s+([0-9.]+)s" % re.escape(label), stderr)
    return float(m.group(1)) if m else None


def is_paste(merged_path, sample_paths):
    """line by line: columns 1-9 of the first per-sample file, then column 10 of each"""
    files = [open(p, "rb") for p in sample_paths]
    try:
        with open(merged_path, "rb") as mf:
            for line in mf:
                rows = [f.readline() for f in files]
                if line.startswith(b"##"):
                    if any(r != line for r in rows):
                        return False
                    continue
                cols = [r.rstrip(b"\n").split(b"\t") for r in rows]
                if line.startswith(b"#CHROM"):
                    continue
                if line != b"\t".join(cols[0][:9] + [c[9] for c in cols]) + b"\n":
                    return False
        return all(f.readline() == b"" for f in files)
    finally:
        for f in files:
            f.close()


def pl_device(a):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from cohort_priors_bench import E, MAX_COV, timed_on, workload
    from malva_amd.capi import Context
    P, n = a.planes, a.records
    dev = torch.device("cuda:0")
    cov, freq, vao = workload(P, n, dev)
    vgo = (3 * torch.arange(n + 1, device=dev, dtype=torch.int64)).contiguous()
    pl = torch.zeros((P, 3 * n), dtype=torch.int32, device=dev)
    plain = [torch.zeros((P, n), dtype=torch.int32, device=dev) for _ in range(3)] + [torch.zeros((P, n), dtype=torch.uint8, device=dev)]
    stream = torch.cuda.Stream()
    res = {"planes": P, "records": n, "alleles": 2, "haploid": 0, "max_cov": MAX_COV, "cap": 255, "repeats": a.repeats, "bytes_moved": P * n * (8 + 12)}
    with torch.cuda.stream(stream), Context(35, 43, 1 << 20) as ctx:
        ctx.set_stream(stream.cuda_stream)
        timed = timed_on(stream)

        def run_plain():
            for p in range(P):
                ctx.genotype_device(cov[p].data_ptr(), freq.data_ptr(), vao.data_ptr(), n, E, MAX_COV, False, plain[0][p].data_ptr(), plain[1][p].data_ptr(),
                                    plain[2][p].data_ptr(), plain[3][p].data_ptr())

        def run_pl():
            ctx.phred_likelihoods_device(n, P, cov.data_ptr(), vao.data_ptr(), vgo.data_ptr(), E, MAX_COV, False, 255, pl.data_ptr())

        legs = {"plain": run_plain, "pl": run_pl}
        for fn in legs.values():                                                   # warm-up: tables, code objects, clocks
            timed(fn)
        ms, own = {leg: [] for leg in legs}, []
        for _ in range(a.repeats):
            for leg, fn in legs.items():
                ms[leg].append(timed(fn))
                if leg == "pl":
                    own.append(ctx.pl_stats())
        stream.synchronize()
        res["cells_best_is_zero"] = round((pl.view(P, n, 3).min(dim=2).values == 0).float().mean().item(), 5)   # (every genotyped cell has a 0)
    res["plain_64_calls_ms"], res["pl_one_call_ms"], res["pl_own_timer_ms"] = stat(ms["plain"]), stat(ms["pl"]), stat(own)
    res["ratio_pl_to_plain"] = round(float(np.median(ms["pl"]) / np.median(ms["plain"])), 3)
    res["pl_gb_per_s"] = round(res["bytes_moved"] / (float(np.median(own)) * 1e-3) / 1e9, 1)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["pl_device"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("cli", "pl_device"), default="cli")
    ap.add_argument("--planes", type=int, default=64, help="--leg pl_device")
    ap.add_argument("--records", type=int, default=1_000_000, help="--leg pl_device")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-gq", type=int, default=20, help="Q of the merged_tags leg")
    ap.add_argument("--parent-bin", default=None, help="malva-geno of the parent commit: its `--cohort -o` panel pass is the yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cohort_merged_bench.json"))
    a = ap.parse_args()
    if a.leg == "pl_device":
        if a.repeats == 3:
            a.repeats = 7
        return pl_device(a)
    S = a.samples
    out = {"workload": "cohort-merged", "k": K, "ref_k": REF_K, "snps": a.snps, "table_rows": a.rows, "samples": S, "repeats": a.repeats}
    panel = synth.flat_from_snp_panel(synth.snp_panel(a.snps, seed=20261016))
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, "c3")
        synth.write_vcf_fasta(panel, prefix)
        hi, lo, _ = synth.flat_kmer_table(panel, a.rows, K, REF_K, seed=7, max_records=min(a.snps, 200_000))
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
        subprocess.run([BIN, "index"] + common + [os.path.join(td, "sample")], check=True, capture_output=True, timeout=600)
        env = dict(os.environ, MALVA_GENO_TIMERS="1")
        legs = {"per_sample": (BIN, ["-o", os.path.join(td, "out")]), "merged": (BIN, ["--merged", os.path.join(td, "merged.vcf")]),
                "merged_tags": (BIN, ["--merged", os.path.join(td, "merged_tags.vcf"), "--min-gq", str(a.min_gq), "--site-tags"]),
                "merged_bcf": (BIN, ["--merged", os.path.join(td, "merged.bcf"), "--merged-format", "bcf"]),
                "merged_ubcf": (BIN, ["--merged", os.path.join(td, "merged.ubcf"), "--merged-format", "ubcf"]),
                "merged_gp": (BIN, ["--merged", os.path.join(td, "merged_gp.vcf"), "--gp"]),
                "merged_gp_bcf": (BIN, ["--merged", os.path.join(td, "merged_gp.bcf"), "--gp", "--merged-format", "bcf"]),
                "merged_pl": (BIN, ["--merged", os.path.join(td, "merged_pl.vcf"), "--pl"]),
                "merged_pl_bcf": (BIN, ["--merged", os.path.join(td, "merged_pl.bcf"), "--pl", "--merged-format", "bcf"])}
        if a.parent_bin:
            legs = dict({"parent": (a.parent_bin, ["-o", os.path.join(td, "out_parent")]),
                         "parent_merged": (a.parent_bin, ["--merged", os.path.join(td, "parent_merged.vcf")]),
                         "parent_merged_bcf": (a.parent_bin, ["--merged", os.path.join(td, "parent_merged.bcf"), "--merged-format", "bcf"])}, **legs)
        res = {leg: {"wall_s": [], "panel_pass_s": []} for leg in legs}
        fmt_ms, fmt_calls = {"merged": [], "merged_tags": [], "merged_gp": [], "merged_pl": [], "parent_merged": []}, 0
        pl_ms, pl_calls = {"merged_pl": [], "merged_pl_bcf": []}, 0
        site_ms, site_calls = [], [0, 0]
        bcf_ms, bcf_calls = {"merged_bcf": [], "merged_ubcf": [], "merged_gp_bcf": [], "merged_pl_bcf": [], "parent_merged_bcf": []}, 0

        def run(leg):
            b, dest = legs[leg]
            t0 = time.perf_counter()
            r = subprocess.run([b, "call", "--cohort"] + dest + common + [os.path.join(td, "cohort.tsv")], capture_output=True, text=True, timeout=1800, env=env)
            wall = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            return wall, r.stderr
        for leg in legs:                                                    # (one run each warms the page cache and the output files' blocks)
            run(leg)
        for _ in range(a.repeats):
            for leg in legs:
                wall, err = run(leg)
                res[leg]["wall_s"].append(wall)
                res[leg]["panel_pass_s"].append(timer(err, "cohort: panel pass"))
                if leg in pl_ms:
                    m = re.search(r"merged: (\d+) mg_phred_likelihoods, device ms per call: ([0-9.]+)", err)
                    pl_calls = int(m.group(1))
                    pl_ms[leg].append(float(m.group(2)))
                if leg in fmt_ms:
                    m = re.search(r"merged: (\d+) mg_format_calls, device ms per call: length ([0-9.]+) scan ([0-9.]+) write ([0-9.]+)", err)
                    fmt_calls = int(m.group(1))
                    fmt_ms[leg].append([float(m.group(i)) for i in (2, 3, 4)])
                if leg in bcf_ms:
                    m = re.search(r"merged: (\d+) mg_encode_calls_bcf, device ms per call: length ([0-9.]+) scan ([0-9.]+) write ([0-9.]+)", err)
                    bcf_calls = int(m.group(1))
                    bcf_ms[leg].append([float(m.group(i)) for i in (2, 3, 4)])
                if leg == "merged_tags":
                    m = re.search(r"merged: (\d+) mg_site_counts, (\d+) mg_format_site_info, device ms per call: count ([0-9.]+) info ([0-9.]+)", err)
                    site_calls = [int(m.group(1)), int(m.group(2))]
                    site_ms.append([float(m.group(3)), float(m.group(4))])
                if leg == "merged":
                    out["merged_timers"] = [l.split("]", 1)[1].strip() for l in err.split("\n") if "timer]" in l and ("cohort" in l or "merged" in l or "worker" in l or "main" in l)]
                if leg == "per_sample":
                    out["per_sample_timers"] = [l.split("]", 1)[1].strip() for l in err.split("\n") if "timer]" in l and ("cohort" in l or "worker" in l or "main" in l)]
        for leg in legs:
            out[leg] = {key: stat(v) for key, v in res[leg].items()}
        out["format_calls_per_run"] = fmt_calls
        out["format_ms_per_call"] = {name: stat([x[i] for x in fmt_ms["merged"]]) for i, name in enumerate(("length", "scan", "write"))}
        out["tags_min_gq"] = a.min_gq
        out["tags_format_ms_per_call"] = {name: stat([x[i] for x in fmt_ms["merged_tags"]]) for i, name in enumerate(("length", "scan", "write"))}
        out["gp_format_ms_per_call"] = {name: stat([x[i] for x in fmt_ms["merged_gp"]]) for i, name in enumerate(("length", "scan", "write"))}
        out["pl_format_ms_per_call"] = {name: stat([x[i] for x in fmt_ms["merged_pl"]]) for i, name in enumerate(("length", "scan", "write"))}
        out["pl_calls_per_run"] = pl_calls
        out["pl_likelihoods_ms_per_call"] = {leg: stat(v) for leg, v in pl_ms.items()}
        if a.parent_bin:
            out["parent_merged_format_ms_per_call"] = {name: stat([x[i] for x in fmt_ms["parent_merged"]]) for i, name in enumerate(("length", "scan", "write"))}
        out["site_calls_per_run"] = {"count": site_calls[0], "info": site_calls[1]}
        out["site_ms_per_call"] = {name: stat([x[i] for x in site_ms]) for i, name in enumerate(("count", "info"))}
        out["encode_calls_per_run"] = bcf_calls
        for leg in bcf_ms:
            if leg not in legs:
                continue
            out[leg + "_encode_ms_per_call"] = {name: stat([x[i] for x in bcf_ms[leg]]) for i, name in enumerate(("length", "scan", "write"))}
        out["merged_bcf_bytes"] = os.path.getsize(os.path.join(td, "merged.bcf"))
        out["merged_ubcf_bytes"] = os.path.getsize(os.path.join(td, "merged.ubcf"))
        out["merged_gp_bytes"] = os.path.getsize(os.path.join(td, "merged_gp.vcf"))
        out["merged_gp_bcf_bytes"] = os.path.getsize(os.path.join(td, "merged_gp.bcf"))
        out["merged_pl_bytes"] = os.path.getsize(os.path.join(td, "merged_pl.vcf"))
        out["merged_pl_bcf_bytes"] = os.path.getsize(os.path.join(td, "merged_pl.bcf"))
        out["merged_tags_bytes"] = os.path.getsize(os.path.join(td, "merged_tags.vcf"))
        out["merged_bytes"] = os.path.getsize(os.path.join(td, "merged.vcf"))
        out["per_sample_bytes"] = sum(os.path.getsize(os.path.join(td, "out", "s%02d.vcf" % i)) for i in range(S))
        out["merged_equals_paste"] = int(is_paste(os.path.join(td, "merged.vcf"), [os.path.join(td, "out", "s%02d.vcf" % i) for i in range(S)]))
        if a.parent_bin:                                                    # per line: medians, the parent's own spread (the margin), the verdict
            out["parent_verdict"] = {}
            for key in ("wall_s", "panel_pass_s"):
                p, t = out["parent"][key], out["per_sample"][key]
                spread = round(p["max"] - p["min"], 3)
                out["parent_verdict"][key] = {"parent_median": p["median"], "parent_spread": spread, "this_median": t["median"],
                                              "within_parent_spread": int(abs(t["median"] - p["median"]) <= spread)}
            out["parent_same_bytes"] =int(all(open(os.path.join(td, "out", "s%02d.vcf" % i), "rb").read() == open(os.path.join(td, "out_parent", "s%02d.vcf" % i), "rb").read()
                                               for i in range(S)))
    if os.path.exists(a.out) and "pl_device" in json.load(open(a.out)):        # (the other leg's result stays)
        out["pl_device"] = json.load(open(a.out))["pl_device"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
