// mg_ibd_step's definition (include/malva_hip.h) as a plain loop on one host core, record by record, over the pairs of the first n_samples samples: what
// tools/ibd_bench.py times beside the device, and compares with it field by field.  Built by that tool with -O2; nothing else uses it.
#include <cstddef>
#include <cstdint>

struct ibd_seg {
    uint32_t a, b, chrom, start_pos, end_pos, n, ibs2, zero;
};

static inline int dosage(const uint64_t *sites, size_t n_vars, size_t v, uint32_t s)
{
    const uint64_t *g = sites + (size_t)(s >> 6) * 3 * n_vars;
    const uint64_t bit = 1ull << (s & 63);
    return g[v] & bit ? 0 : g[n_vars + v] & bit ? 1 : g[2 * n_vars + v] & bit ? 2 : -1;
}

// the whole table of one walk with a flush behind the last record, ordered by (a, b, start) -> the segments needed; the first `cap` are written
extern "C" uint64_t ibd_walk_host(size_t n_vars, uint32_t n_samples, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, uint32_t min_records, int64_t min_bp,
                                  ibd_seg *segs, size_t cap)
{
    uint64_t k = 0;
    for (uint32_t a = 0; a < n_samples; ++a)
        for (uint32_t b = a + 1; b < n_samples; ++b) {
            bool open = false;
            uint32_t c = 0, start = 0, end = 0, n = 0, ibs2 = 0;
            auto close = [&] {
                if (open && n >= min_records && (int64_t)end - (int64_t)start >= min_bp) {
                    if (k < cap) segs[k] = ibd_seg{a, b, c, start, end, n, ibs2, 0};
                    ++k;
                }
                open = false;
            };
            for (size_t v = 0; v < n_vars; ++v) {
                if (open && chrom[v] != c) close();
                const int da = dosage(sites, n_vars, v, a), db = dosage(sites, n_vars, v, b);
                if (da < 0 || db < 0) continue;
                if (da + db == 2 && da != db) {
                    close();
                    continue;
                }
                if (!open) open = true, c = chrom[v], start = pos[v], n = ibs2 = 0;
                end = pos[v], ++n, ibs2 += da == db;
            }
            close();
        }
    return k;
}
