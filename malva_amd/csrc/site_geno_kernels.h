// The per-record QC of a multi-sample call set made on the device: per record and allele the genotype counts over the planes of a cohort
// (mg_site_geno_counts_device), and per (record, ALT) the exact test of Hardy-Weinberg proportions (mg_hwe_exact_device).  The reference --
// one individual per run -- has neither.
//
// Counts: site_geno_kernel, one wave per record, lane = plane, the shape of site_count_kernel.  A cell is USABLE when it is not masked
// (the mask on and gq < min_gq) and every allele index the mode reads lies in [0, A); a cell that is not stands as the index pair (~0, ~0),
// which no allele matches.  A usable cell with gt1 == gt2 (haploid: always) is one homozygote of slot gt1, one with gt1 != gt2 one heterozygote
// of slot gt1 and one of slot gt2.  Records of up to SITE_BALLOT_MAX alleles count a slot by two ballots; records with more go through two
// histograms of the wave's own in LDS, SITE_BINS alleles at a time.  A record belongs to one wave: `accumulate` adds without atomics.
//
// Test: hwe_exact_kernel, one thread per item, every step one correctly rounded f64 operation in the order mg_hwe_exact's comment in
// malva_hip.h fixes (the library is built with -ffp-contract=off; f64 subnormals are kept).  No per-item array: one walk from the mode
// to the observed count finds q_obs, a second one makes the three sums.  A wave per item would change the order of the sums.
#pragma once
#include "site_tags_kernels.h"

namespace {
using namespace mg;

constexpr int HWE_TPB = 64; // items differ in length by orders of magnitude: small workgroups, so that a long item holds few others back

__global__ void __launch_bounds__(FMT_TPB) site_geno_kernel(SiteArgs a, u32 *__restrict__ n_out, u32 *__restrict__ het, u32 *__restrict__ hom)
{
    __shared__ u32 hist[FMT_TPB / 64][2][SITE_BINS];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 v = (u64)blockIdx.x * (FMT_TPB / 64) + wave;
    if (v >= a.n_vars) return; // (wave-uniform)
    const u32 a0 = a.var_allele_off[v], A = a.var_allele_off[v + 1] - a0;
    bool usable = lane < a.n_planes;
    u32 g1 = ~0u, g2 = ~0u;
    if (usable) {
        const u64 i = (u64)lane * a.n_vars + v;
        g1 = (u32)a.gt1[i];
        g2 = a.haploid ? g1 : (u32)a.gt2[i];
        if (a.use_mask) usable = a.gq[i] >= a.min_gq;
    }
    usable = usable && g1 < A && g2 < A; // (a negative index is a large unsigned one)
    if (!usable) g1 = g2 = ~0u;
    const u32 n_usable = (u32)__popcll(__ballot(usable));
    if (lane == 0) n_out[v] = (a.accumulate ? n_out[v] : 0u) + n_usable;
    if (A <= SITE_BALLOT_MAX) {
        u32 my_het = 0, my_hom = 0;
        for (u32 al = 0; al < A; ++al) {
            const bool in = g1 == al || g2 == al;
            const u32 n_hom = (u32)__popcll(__ballot(in && g1 == g2)), n_het = (u32)__popcll(__ballot(in && g1 != g2));
            if (lane == al) my_hom = n_hom, my_het = n_het;
        }
        if (lane < A) {
            het[a0 + lane] = (a.accumulate ? het[a0 + lane] : 0u) + my_het;
            hom[a0 + lane] = (a.accumulate ? hom[a0 + lane] : 0u) + my_hom;
        }
        return;
    }
    u32 *h_het = hist[wave][0], *h_hom = hist[wave][1]; // the wave's own: its LDS operations complete in program order, no other wave touches the rows
    for (u32 base = 0; base < A; base += SITE_BINS) {
        const u32 top = A - base < SITE_BINS ? A - base : SITE_BINS;
        h_het[lane] = h_het[lane + 64] = 0;
        h_hom[lane] = h_hom[lane + 64] = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (g1 == g2) {
            if (g1 - base < top) atomicAdd(&h_hom[g1 - base], 1u);
        } else {
            if (g1 - base < top) atomicAdd(&h_het[g1 - base], 1u);
            if (g2 - base < top) atomicAdd(&h_het[g2 - base], 1u);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (u32 k = lane; k < top; k += 64) {
            het[a0 + base + k] = (a.accumulate ? het[a0 + base + k] : 0u) + h_het[k];
            hom[a0 + base + k] = (a.accumulate ? hom[a0 + base + k] : 0u) + h_hom[k];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// one step of the walk: the ratio first, from two exact integers, then the product (a ratio of exactly 1 keeps q bit for bit)
__device__ __forceinline__ double hwe_down(double q, u64 h, u64 hr, u64 hc) { return q * ((double)(h * (h - 1)) / (double)(4 * (hr + 1) * (hc + 1))); }
__device__ __forceinline__ double hwe_up(double q, u64 h, u64 hr, u64 hc) { return q * ((double)(4 * hr * hc) / (double)((h + 2) * (h + 1))); }

__global__ void __launch_bounds__(HWE_TPB) hwe_exact_kernel(u64 n_items, const u32 *__restrict__ n_in, const u32 *__restrict__ het_in, const u32 *__restrict__ hom_in,
                                                            double *__restrict__ hwe_out, double *__restrict__ exc_out)
{
    const u64 i = (u64)blockIdx.x * HWE_TPB + threadIdx.x;
    if (i >= n_items) return;
    const u64 n = n_in[i], het = het_in[i], hom = hom_in[i];
    if (het + hom > n || n > MG_HWE_MAX_N) {
        hwe_out[i] = exc_out[i] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const u64 na = het + 2 * hom, nb = 2 * n - na, r = na < nb ? na : nb;
    u64 mid = n ? r * (2 * n - r) / (2 * n) : 0;
    if ((mid ^ r) & 1) ++mid;
    const u64 hr0 = (r - mid) / 2, hc0 = n - mid - hr0;
    double q_obs = 1.0;
    {
        u64 h = mid, hr = hr0, hc = hc0;
        for (; h > het; h -= 2, ++hr, ++hc) q_obs = hwe_down(q_obs, h, hr, hc);
        for (; h < het; h += 2, --hr, --hc) q_obs = hwe_up(q_obs, h, hr, hc);
    }
    double S = 1.0, L = 1.0 <= q_obs ? 1.0 : 0.0, G = mid >= het ? 1.0 : 0.0, q = 1.0;
    u64 h = mid, hr = hr0, hc = hc0;
    while (h > 1) {
        q = hwe_down(q, h, hr, hc);
        h -= 2, ++hr, ++hc;
        S += q;
        if (q <= q_obs) L += q;
        if (h >= het) G += q;
    }
    q = 1.0, h = mid, hr = hr0, hc = hc0;
    while (h + 2 <= r) {
        q = hwe_up(q, h, hr, hc);
        h += 2, --hr, --hc;
        S += q;
        if (q <= q_obs) L += q;
        if (h >= het) G += q;
    }
    const double p = L / S, e = G / S;
    hwe_out[i] = p < 1.0 ? p : 1.0;
    exc_out[i] = e < 1.0 ? e : 1.0;
}

} // namespace
