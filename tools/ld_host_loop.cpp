// mg_ld_window's definition (include/malva_hip.h) as a plain loop on one host core: what tools/ld_bench.py times beside the device, and compares
// with it bit for bit.  Built by that tool with -O2 -mpopcnt -ffp-contract=off; nothing else uses it.
#include <cstddef>
#include <cstdint>

struct ld_pair {
    uint32_t i, j, n;
    int32_t sign;
    double r2;
};

// -> the pairs needed; the first `cap` of them are written, row_off [n_first + 1] always
extern "C" uint64_t ld_window_host(size_t n_vars, size_t n_first, uint32_t n_groups, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, uint32_t window,
                                   uint64_t max_bp, uint32_t min_n, double min_r2, ld_pair *pairs, size_t cap, uint64_t *row_off)
{
    uint64_t k = 0;
    for (size_t i = 0; i < n_first; ++i) {
        row_off[i] = k;
        for (size_t j = i + 1; j <= i + window && j < n_vars; ++j) {
            if (chrom[i] != chrom[j]) continue;
            const long long d = (long long)pos[j] - (long long)pos[i];
            if (max_bp && (uint64_t)(d < 0 ? -d : d) > max_bp) continue;
            long long n = 0, x1 = 0, x2 = 0, y1 = 0, y2 = 0, sxy = 0;
            for (uint32_t g = 0; g < n_groups; ++g) {
                const uint64_t *s = sites + (size_t)g * 3 * n_vars;
                const uint64_t a0 = s[i], a1 = s[n_vars + i], a2 = s[2 * n_vars + i], b0 = s[j], b1 = s[n_vars + j], b2 = s[2 * n_vars + j];
                const uint64_t A = a0 | a1 | a2, B = b0 | b1 | b2;
                n += __builtin_popcountll(A & B);
                x1 += __builtin_popcountll(a1 & B), x2 += __builtin_popcountll(a2 & B);
                y1 += __builtin_popcountll(A & b1), y2 += __builtin_popcountll(A & b2);
                sxy += __builtin_popcountll(a1 & b1) + 2 * (__builtin_popcountll(a1 & b2) + __builtin_popcountll(a2 & b1)) + 4 * __builtin_popcountll(a2 & b2);
            }
            const long long sx = x1 + 2 * x2, sxx = x1 + 4 * x2, sy = y1 + 2 * y2, syy = y1 + 4 * y2;
            const long long cov = n * sxy - sx * sy, vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
            if (n < (long long)min_n || vx <= 0 || vy <= 0) continue;
            const double r2 = (double)(uint64_t)(cov * cov) / (double)(uint64_t)(vx * vy);
            if (!(r2 >= min_r2)) continue;
            if (k < cap) pairs[k] = ld_pair{(uint32_t)i, (uint32_t)j, (uint32_t)n, cov > 0 ? 1 : cov < 0 ? -1 : 0, r2};
            ++k;
        }
    }
    row_off[n_first] = k;
    return k;
}
