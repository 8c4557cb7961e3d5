"""The two kernels behind `call --cohort --pairs` on one MI355X, through the C ABI: mg_pack_dosage and mg_pair_counts on 64 planes
x 1e6 records -- the records of a synthetic SNP panel (malva_amd/synth.py: all biallelic), calls drawn at its allele frequencies
with a few indexes outside {0, 1}, GQ on both sides of the mask.

Reported, each the median of --repeats calls with their spread (device milliseconds from mg_pairs_stats: the kernels alone, no copy):
    pack    the bytes it must move -- 12 B per cell read (gt1, gt2, gq), 8 B per record of var_allele_off, 3 bits per cell written --
            and the rate that follows
    count   B == A, the whole square: the bytes it must read once, (n_a + n_b) * 3 * 8 * W, the AND+popcount operations on 64-bit
            words it performs -- 9 per word and pair it computes, the pairs of the tiles on and above the diagonal -- and the rate
            that follows; the same for the definition's n_a * n_b * 9 * W
    count_ab  A against a second group of as many planes (the pass over pairs of groups): every tile is computed
The counts are compared with numpy on the first --check-words words.

    python tools/pairs_bench.py [--planes 64] [--records 1000000] [--repeats 5] [--out profiles/pairs_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from malva_amd import Context, synth  # noqa: E402

TILE = 16  # PAIR_TILE of csrc/pair_kernels.h


def stat(xs):
    xs = sorted(xs)
    return {"median": round(float(np.median(xs)), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def popcount_pairs(a, b):
    bits = lambda p: np.unpackbits(np.ascontiguousarray(p, dtype="<u8").view(np.uint8).reshape(p.shape[0], 3, -1), axis=-1, bitorder="little").astype(np.float64)
    return np.einsum("idw,jew->ijde", bits(a), bits(b), optimize=True).round().astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-gq", type=int, default=20)
    ap.add_argument("--check-words", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_bench.json"))
    a = ap.parse_args()
    P, n = a.planes, a.records
    W = (n + 63) // 64
    panel = synth.snp_panel(n, seed=20261018)
    vao = np.ascontiguousarray(panel.var_allele_off, dtype=np.uint32)
    assert vao.size == n + 1
    rng = np.random.default_rng(7)
    af = rng.beta(0.5, 2.0, size=n)

    def draw():
        g = (rng.random((P, n)) < af[None, :]).astype(np.int32)
        g[rng.random((P, n)) < 0.01] = -1
        return g
    g1, g2 = draw(), draw()
    gq = rng.integers(0, 60, size=(P, n)).astype(np.int32)
    out = {"workload": "pairs", "planes": P, "records": n, "words": W, "repeats": a.repeats, "min_gq": a.min_gq}
    with Context(35, 43, 1 << 20) as c:
        planes = None
        pack_ms, count_ms, cross_ms = [], [], []
        for _ in range(a.repeats + 1):                                       # (the first call allocates: not kept)
            planes = c.pack_dosage(g1, g2, gq, False, vao, min_gq=a.min_gq, out=planes)
            pack_ms.append(c.pairs_stats()[0])
        other = np.ascontiguousarray(planes[::-1])
        for _ in range(a.repeats + 1):
            counts = c.pair_counts(planes)
            count_ms.append(c.pairs_stats()[1])
            cross = c.pair_counts(planes, other)
            cross_ms.append(c.pairs_stats()[1])
        k = min(W, a.check_words)
        out["check_words"] = k
        out["counts_equal_numpy"] = int(np.array_equal(c.pair_counts(planes[:, :, :k]), popcount_pairs(planes[:, :, :k], planes[:, :, :k])) and
                                        np.array_equal(c.pair_counts(planes[:, :, :k], other[:, :, :k]), popcount_pairs(planes[:, :, :k], other[:, :, :k])) and
                                        np.array_equal(cross, counts[:, ::-1]))
    out["called_cells"] = int(counts[np.arange(P), np.arange(P)].sum())
    out["pack_ms"], out["count_ms"], out["count_ab_ms"] = stat(pack_ms[1:]), stat(count_ms[1:]), stat(cross_ms[1:])
    pack_bytes = 12 * P * n + 4 * (n + 1) * P + 8 * 3 * P * W                # (every wave reads its records' var_allele_off: once per plane)
    out["pack_bytes"] = pack_bytes
    out["pack_gb_per_s"] = round(pack_bytes / out["pack_ms"]["median"] / 1e6, 1)
    tiles = (P + TILE - 1) // TILE
    out["count_bytes_read_once"] = 2 * P * 3 * 8 * W
    for key, ms, pairs in (("count", out["count_ms"], tiles * (tiles + 1) // 2 * TILE * TILE), ("count_ab", out["count_ab_ms"], tiles * tiles * TILE * TILE)):
        out[key + "_and_popcount_ops"] = 9 * pairs * W
        out[key + "_gops_per_s"] = round(9 * pairs * W / ms["median"] / 1e6, 1)
    out["count_defined_ops"] = 9 * P * P * W
    out["count_defined_gops_per_s"] = round(9 * P * P * W / out["count_ms"]["median"] / 1e6, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
