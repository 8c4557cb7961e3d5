"""mg_pca_solve on one MI355X: the principal components of a synthetic three-population genetic relationship matrix at n = 1,024, 4,096
and 16,384 samples.

The matrix is the one of tests/pca_cases.py (grm_like) at a larger size: three populations of n / 3 samples (the last takes the remainder),
binomial genotypes over --records records at frequencies drifted by F = 0.05 from a common one, standardised per record, G = Z Z^T / records
(the product is made on the device with torch, in float64), rounded to float32 as GCTA's .grm.bin holds it.  It is loaded once per size
(mg_pca_load_f64) and solved at K = 2 and K = 20, tol 1e-10, at most --max-iters products, --repeats times; reported per run: the products,
the pairs converged, and the medians of mg_pca_stats' device milliseconds (products, orthonormalisation, Rayleigh-Ritz with the host's
small solver, total), the milliseconds and bytes per second of one product, and at 1,024 and 4,096 the wall time of numpy.linalg.eigh on
the same matrix with the largest difference between its leading eigenvalues and the device's.
EXPECTATIONS, written before any run.  A product streams G once: 8 n'^2 bytes (2.1 GB at 16,384) and should run at half the HBM rate of
8 TB/s or better, about 0.5 ms at 16,384; at 78 TF of f64 matrix rate its 2 n^2 m flops take less than that, so the kernel should be bound
by the stream of G.  How many products the components inside the bulk need at 16,384 nobody has measured; a CPU prototype needed 12-16 for
separated components and 100-260 for components inside the bulk at n = 200 and 600.

    python tools/pca_bench.py [--sizes 1024,4096,16384] [--records 5000] [--repeats 5] [--max-iters 2000] [--out profiles/pca_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from malva_amd import Context  # noqa: E402

HBM_BYTES_PER_S = 8e12
F64_MATRIX_FLOPS = 78e12


def three_populations(n, n_records, F=0.05, seed=7):
    """-> G float64 [n, n] holding float32 values"""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(0.1, 0.9, size=n_records)
    a, b = p0 * (1 - F) / F, (1 - p0) * (1 - F) / F
    sizes = [n // 3, n // 3, n - 2 * (n // 3)]
    X = np.concatenate([rng.binomial(2, rng.beta(a, b)[None, :], size=(s, n_records)).astype(np.int8) for s in sizes])
    ph = X.mean(axis=0, dtype=np.float64) / 2
    keep = (ph > 0.01) & (ph < 0.99)
    dev = torch.device("cuda", 0)
    Z = torch.from_numpy(X[:, keep]).to(dev).to(torch.float64)
    phd = torch.from_numpy(ph[keep]).to(dev)
    Z = (Z - 2 * phd[None, :]) / torch.sqrt(2 * phd * (1 - phd))[None, :]
    G = (Z @ Z.T) / Z.shape[1]
    G = torch.tril(G).to(torch.float32).to(torch.float64)
    G = G + torch.tril(G, -1).T
    return G.cpu().numpy()


def med(xs):
    return round(float(np.median(xs)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--records", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=2000)
    ap.add_argument("--eigh-up-to", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_bench.json"))
    o = ap.parse_args()
    runs = []
    with Context(35, 43, 1 << 20) as ctx:
        for n in [int(x) for x in o.sizes.split(",")]:
            G = three_populations(n, o.records)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            t0 = time.perf_counter()
            ctx.pca_load(G)
            load_s = time.perf_counter() - t0
            ref = None
            if n <= o.eigh_up_to:
                t0 = time.perf_counter()
                w = np.linalg.eigh(G)[0][::-1]
                ref = {"eigh_wall_s": round(time.perf_counter() - t0, 3), "values": w}
            np_pad = (n + 15) // 16 * 16
            for k in (2, 20):
                ms, products, converged, wall, values, m = [], [], [], [], None, 0
                for _ in range(o.repeats):
                    t0 = time.perf_counter()
                    values, _, resid, scale, info = ctx.pca_solve(n, k, 1e-10, o.max_iters)
                    wall.append(time.perf_counter() - t0)
                    ms.append(ctx.pca_stats())
                    products.append(info[0])
                    converged.append(info[1])
                    m = info[2]
                ms = np.array(ms)
                per_product = float(np.median(ms[:, 0] / np.maximum(1, products)))
                run = {"n": n, "k": k, "m": m, "records": o.records, "products": int(np.median(products)), "converged": int(np.median(converged)), "max_iters": o.max_iters,
                       "ms_products": med(ms[:, 0]), "ms_orthonormalise": med(ms[:, 1]), "ms_rayleigh_ritz": med(ms[:, 2]), "ms_total": med(ms[:, 3]),
                       "wall_s": med(wall), "ms_per_product": round(per_product, 4), "bytes_per_product": 8 * np_pad * np_pad,
                       "tb_per_s": round(8 * np_pad * np_pad / (per_product * 1e-3) / 1e12, 3) if per_product > 0 else None,
                       "expected_ms_per_product_at_half_hbm": round(8 * np_pad * np_pad / (HBM_BYTES_PER_S / 2) * 1e3, 4),
                       "flops_ms_at_f64_matrix_rate": round(2.0 * np_pad * np_pad * m / F64_MATRIX_FLOPS * 1e3, 4),
                       "load_wall_s": round(load_s, 3), "max_residual": float(resid.max())}
                if ref is not None:
                    run["eigh_wall_s"] = ref["eigh_wall_s"]
                    run["max_abs_diff_to_eigh"] = float(np.abs(values - ref["values"][:k]).max())
                runs.append(run)
                print(json.dumps(run), flush=True)
            ctx.pca_end()
    result = {"tool": "tools/pca_bench.py", "device": torch.cuda.get_device_name(0), "repeats": o.repeats, "runs": runs}
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
