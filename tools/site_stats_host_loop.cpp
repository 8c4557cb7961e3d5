// mg_hwe_exact's definition (include/malva_hip.h) as a plain loop on one host core: what tools/site_stats_bench.py times beside the device, and
// compares with it bit for bit.  Built by that tool with -O2 -ffp-contract=off; nothing else uses it.
#include <cmath>
#include <cstddef>
#include <cstdint>

static inline double down(double q, uint64_t h, uint64_t hr, uint64_t hc) { return q * ((double)(h * (h - 1)) / (double)(4 * (hr + 1) * (hc + 1))); }
static inline double up(double q, uint64_t h, uint64_t hr, uint64_t hc) { return q * ((double)(4 * hr * hc) / (double)((h + 2) * (h + 1))); }

extern "C" void hwe_exact_host(size_t n_items, const uint32_t *n_in, const uint32_t *het_in, const uint32_t *hom_in, double *hwe_out, double *exc_out)
{
    for (size_t i = 0; i < n_items; ++i) {
        const uint64_t n = n_in[i], het = het_in[i], hom = hom_in[i];
        if (het + hom > n || n > (1u << 24)) {
            hwe_out[i] = exc_out[i] = NAN;
            continue;
        }
        const uint64_t na = het + 2 * hom, nb = 2 * n - na, r = na < nb ? na : nb;
        uint64_t mid = n ? r * (2 * n - r) / (2 * n) : 0;
        if ((mid ^ r) & 1) ++mid;
        const uint64_t hr0 = (r - mid) / 2, hc0 = n - mid - hr0;
        double q_obs = 1.0;
        uint64_t h = mid, hr = hr0, hc = hc0;
        for (; h > het; h -= 2, ++hr, ++hc) q_obs = down(q_obs, h, hr, hc);
        for (; h < het; h += 2, --hr, --hc) q_obs = up(q_obs, h, hr, hc);
        double S = 1.0, L = 1.0 <= q_obs ? 1.0 : 0.0, G = mid >= het ? 1.0 : 0.0, q = 1.0;
        h = mid, hr = hr0, hc = hc0;
        while (h > 1) {
            q = down(q, h, hr, hc);
            h -= 2, ++hr, ++hc;
            S += q;
            if (q <= q_obs) L += q;
            if (h >= het) G += q;
        }
        q = 1.0, h = mid, hr = hr0, hc = hc0;
        while (h + 2 <= r) {
            q = up(q, h, hr, hc);
            h += 2, --hr, --hc;
            S += q;
            if (q <= q_obs) L += q;
            if (h >= het) G += q;
        }
        const double p = L / S, e = G / S;
        hwe_out[i] = p < 1.0 ? p : 1.0;
        exc_out[i] = e < 1.0 ? e : 1.0;
    }
}
