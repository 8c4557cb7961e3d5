// mg_grm_step's definition (include/malva_hip.h) as a plain loop on one host core: the records' weights, then every pair a <= b of the first n_pairs_of
// samples record by record.  What tools/grm_bench.py times beside the device and compares with it value by value (built by that tool with -O2
// -ffp-contract=off), and what stands in for the device in tools/grm_out_host_check.cpp.
#include <cmath>
#include <cstddef>
#include <cstdint>

static inline int grm_dosage(const uint64_t *sites, size_t n_vars, size_t v, uint32_t s, uint32_t n_samples, int haploid)
{
    if (s >= n_samples) return -1;
    const uint64_t *g = sites + (size_t)(s >> 6) * 3 * n_vars;
    const uint64_t bit = 1ull << (s & 63);
    return g[v] & bit ? 0 : !haploid && (g[n_vars + v] & bit) ? 1 : g[2 * n_vars + v] & bit ? 2 : -1;
}

// one record's weights over all n_samples samples: q[0..2], and whether it enters
static inline bool grm_record_weights(const uint64_t *sites, size_t n_vars, size_t v, uint32_t n_samples, int haploid, uint32_t maf_ppm, uint32_t min_n, int64_t q[3])
{
    int64_t cnt[3] = {0, 0, 0};
    for (uint32_t s = 0; s < n_samples; ++s) {
        const int d = grm_dosage(sites, n_vars, v, s, n_samples, haploid);
        if (d >= 0) ++cnt[d];
    }
    const int64_t n = haploid ? cnt[0] + cnt[2] : cnt[0] + cnt[1] + cnt[2], an = haploid ? n : 2 * n, ac = haploid ? cnt[2] : cnt[1] + 2 * cnt[2];
    const int64_t D = (haploid ? 4 : 2) * ac * (an - ac);
    q[0] = q[1] = q[2] = 0;
    if (D <= 0) return false;
    const double root = std::sqrt((double)D);
    bool fits = true;
    for (int d = 0; d < 3; ++d) {
        q[d] = (int64_t)std::nearbyint((double)((d * an - 2 * ac) * 1024) / root); // (the default rounding mode: half to even)
        fits = fits && q[d] <= 32639 && q[d] >= -32639;
    }
    const int64_t minor = ac < an - ac ? ac : an - ac;
    return fits && n >= (int64_t)min_n && (uint64_t)minor * 1000000ull >= (uint64_t)maf_ppm * (uint64_t)an;
}

// adds n_vars records to sum / count, [n_samples (n_samples + 1) / 2], pair (a, b) at a (2 n - a + 1) / 2 + b - a; only the pairs with a < first_rows
// are formed (the benchmark's slice; n_samples for all of them).  -> the records that entered
extern "C" uint64_t grm_step_host(size_t n_vars, uint32_t n_samples, const uint64_t *sites, int haploid, uint32_t maf_ppm, uint32_t min_n, uint32_t first_rows,
                                  int64_t *sum, uint64_t *count)
{
    uint64_t entered = 0;
    for (size_t v = 0; v < n_vars; ++v) {
        int64_t q[3];
        if (!grm_record_weights(sites, n_vars, v, n_samples, haploid, maf_ppm, min_n, q)) continue;
        ++entered;
        for (uint32_t a = 0; a < n_samples && a < first_rows; ++a) {
            const int da = grm_dosage(sites, n_vars, v, a, n_samples, haploid);
            if (da < 0) continue;
            size_t k = (size_t)a * (2 * (size_t)n_samples - a + 1) / 2;
            for (uint32_t b = a; b < n_samples; ++b, ++k) {
                const int db = grm_dosage(sites, n_vars, v, b, n_samples, haploid);
                if (db < 0) continue;
                sum[k] += q[da] * q[db];
                ++count[k];
            }
        }
    }
    return entered;
}
