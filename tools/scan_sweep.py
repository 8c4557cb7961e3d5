#!/usr/bin/env python3
"""A/B the scan kernels' launch parameters in ONE process on one index and one table
(cdna_hip_programming.md rule 24): interleaved rounds, median + min per variant.
usage: python tools/scan_sweep.py [--kmers 1e8] [--variants 1e6] opt=v1,v2 [opt2=...]
Index-time options (gate_*: set before any insert) may take several values too: the index is then built once per
combination of them over the same panel and table, the launch parameters swept on each."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from malva_amd import BF_ALT, BF_CTX, Context, synth  # noqa: E402


def main():
    args = sys.argv[1:]
    n_rows, n_vars, b, rounds, compact = int(1e8), int(1e6), 4, 7, False
    sweeps = {}
    while args:
        a = args.pop(0)
        if a == "--kmers":
            n_rows = int(float(args.pop(0)))
        elif a == "--variants":
            n_vars = int(float(args.pop(0)))
        elif a == "--b":
            b = int(args.pop(0))
        elif a == "--rounds":
            rounds = int(args.pop(0))
        elif a == "--compact":      # 12-byte packed rows (scan_filter12_kernel: what bench.py's C3 step runs)
            compact = True
        else:
            k, v = a.split("=")
            sweeps[k] = [int(x) for x in v.split(",")]
    K, R = 35, 43
    dev = torch.device("cuda", 0)
    panel = synth.snp_panel(n_vars, seed=20261003)
    sig, _ = synth.snp_signature_rows(panel, K)
    rows = np.zeros((sig.shape[0], 40), dtype=np.uint8)
    rows[:, :K] = sig
    hi, lo, cnt = synth.kmer_table(panel, n_rows, K, R, seed=777)
    d_hi = torch.from_numpy(hi.view(np.int64)).to(dev)
    d_lo = torch.from_numpy(lo.view(np.int64)).to(dev)
    d_cnt = torch.from_numpy(cnt.view(np.int32)).to(dev)
    index_keys = [k for k in sweeps if k.startswith("gate_")]      # index-time options: before any insert
    index_combos = list(itertools.product(*[sweeps.pop(k) for k in index_keys])) or [()]
    keys = list(sweeps)
    combos = list(itertools.product(*[sweeps[k] for k in keys])) or [()]
    ref, d_rows = None, None
    for ic in index_combos:
        ctx = Context(K, R, b << 33)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for k, v in zip(index_keys, ic):
            ctx.set_option(k, v)
        ctx.map_insert(rows[0::2]); ctx.bf_insert(BF_ALT, rows[1::2]); ctx.bf_finalize(BF_ALT)
        ctx.ref_scan(panel.genome.tobytes()); ctx.bf_finalize(BF_CTX)
        if compact and d_rows is None:
            d_rows = torch.zeros(ctx.kmc_rows_bytes(n_rows) // 4, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.kmc_pack_rows_device(d_hi.data_ptr(), d_lo.data_ptr(), d_cnt.data_ptr(), n_rows, d_rows.data_ptr())
            ctx.synchronize()
        times = {c: [] for c in combos}
        for rnd in range(rounds + 1):
            for c in combos:
                for k, v in zip(keys, c):
                    ctx.set_option(k, v)
                ctx.counters_reset()
                if compact:
                    ctx.kmc_scan_rows_device(d_rows.data_ptr(), n_rows)
                else:
                    ctx.kmc_scan_device(d_hi.data_ptr(), d_lo.data_ptr(), d_cnt.data_ptr(), n_rows)
                f, pr, h, n_open, nh = ctx.scan_stats()
                if rnd:
                    times[c].append((f, pr, h, n_open, nh))
                else:   # results must depend neither on the launch parameters nor on the gate's geometry
                    d = torch.zeros(sum(ctx.counters_size()), dtype=torch.int32, device=dev)
                    ctx.counters_export_device(d.data_ptr()); ctx.synchronize()
                    ref = d if ref is None else ref
                    assert "scan_ablate" in keys or torch.equal(ref, d), "counters differ for %s %s" % (ic, c)
        for c in combos:
            f = np.array([t[0] for t in times[c]]); pr = np.array([t[1] for t in times[c]]); h = np.array([t[2] for t in times[c]])
            label = dict(zip(index_keys + keys, ic + c))
            if index_keys:
                label["gate_words"] = ctx.get_option("gate_words")
            print("%-36s filter median %.3f min %.3f | probe %.3f | hits %.3f ms | open %d hit %d | filter %.3g kmers/s, all %.3g" %
                  (label, np.median(f), f.min(), np.median(pr), np.median(h), times[c][-1][3], times[c][-1][4],
                   n_rows / (np.median(f) * 1e-3), n_rows / (np.median(f + pr + h) * 1e-3)), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
