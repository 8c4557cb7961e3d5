// The site tags of a multi-sample VCF made on the device: per record the allele counts over the planes of a cohort, and the INFO
// string `AC=a1,a2,..;AN=n;AF=f1,f2,..;NS=s` they give.  The reference -- one individual per run -- has neither.
//
// Counts (mg_site_counts_device): site_count_kernel, one wave per record, lane = plane, the shape of fmt_len_kernel.  A cell is
// called unless the mask is on and its gq < min_gq; a called cell adds one copy of gt1 and, diploid, one of gt2 to the record's
// slots ac[var_allele_off[v] + allele] (REF is allele 0) and one to ns[v].  Records of up to SITE_BALLOT_MAX alleles count an allele
// as popcount(ballot(gt1 == a)) + popcount(ballot(gt2 == a)); records with more go through a histogram of the wave's own in LDS,
// SITE_BINS alleles at a time.  An index outside the record's alleles is not counted.  A record belongs to one wave: `accumulate`
// adds to what the slots hold without atomics.
//
// INFO text (mg_format_site_info_device): the three steps of mg_format_calls -- info_len_kernel, the same scan, info_write_kernel
// (fmt_write_tile of call_text_kernels.h) -- with the lanes of a record's wave over its alleles.  site_info_row lays a row out for
// both passes, so that the lengths and the bytes cannot disagree.  AN is the sum of the record's slots; AF_i = AC_i / AN rounded
// half up to six decimals in integers: q = (2 AC 10^6 + AN) / (2 AN); 0 prints `0`, 10^6 prints `1`, anything else `0.` and six
// zero-padded digits without their trailing zeros; AN = 0 prints `.`.  A record without ALT alleles prints `AN=n;NS=s`.
#pragma once
#include "call_text_kernels.h"

namespace {
using namespace mg;

constexpr u32 SITE_BALLOT_MAX = 8; // alleles per record counted by ballots (two ballots each: beyond this the histogram is cheaper)
constexpr u32 SITE_BINS = 128;     // histogram bins per wave: the alleles the panel's 7-bit genotype packing admits, in one round

struct SiteArgs {
    u64 n_vars;
    u32 n_planes;
    int haploid;
    const i32 *gt1, *gt2, *gq; // [n_planes][n_vars]
    int use_mask;
    i32 min_gq;
    const u32 *var_allele_off; // [n_vars + 1]
    int accumulate;
};

__global__ void __launch_bounds__(FMT_TPB) site_count_kernel(SiteArgs a, u32 *__restrict__ ac, u32 *__restrict__ ns)
{
    __shared__ u32 hist[FMT_TPB / 64][SITE_BINS];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 v = (u64)blockIdx.x * (FMT_TPB / 64) + wave;
    if (v >= a.n_vars) return; // (wave-uniform)
    const u32 a0 = a.var_allele_off[v], A = a.var_allele_off[v + 1] - a0;
    bool called = lane < a.n_planes;
    u32 g1 = ~0u, g2 = ~0u; // (an index no record has)
    if (called) {
        const u64 i = (u64)lane * a.n_vars + v;
        g1 = (u32)a.gt1[i];
        if (!a.haploid) g2 = (u32)a.gt2[i];
        if (a.use_mask) called = a.gq[i] >= a.min_gq;
    }
    if (!called) g1 = g2 = ~0u;
    const u32 n_called = (u32)__popcll(__ballot(called));
    if (lane == 0) ns[v] = (a.accumulate ? ns[v] : 0u) + n_called;
    if (A <= SITE_BALLOT_MAX) {
        u32 mine = 0;
        for (u32 al = 0; al < A; ++al) {
            const u32 n = (u32)__popcll(__ballot(g1 == al)) + (u32)__popcll(__ballot(g2 == al));
            if (lane == al) mine = n;
        }
        if (lane < A) ac[a0 + lane] = (a.accumulate ? ac[a0 + lane] : 0u) + mine;
        return;
    }
    u32 *h = hist[wave]; // the wave's own: its LDS operations complete in program order, no other wave touches the row
    for (u32 base = 0; base < A; base += SITE_BINS) {
        const u32 top = A - base < SITE_BINS ? A - base : SITE_BINS;
        h[lane] = 0;
        h[lane + 64] = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (g1 - base < top) atomicAdd(&h[g1 - base], 1u);
        if (g2 - base < top) atomicAdd(&h[g2 - base], 1u);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (u32 k = lane; k < top; k += 64) ac[a0 + base + k] = (a.accumulate ? ac[a0 + base + k] : 0u) + h[k];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

struct InfoArgs {
    u64 n_vars;
    const u32 *ac;             // [var_allele_off[n_vars]]
    const u32 *ns;             // [n_vars]
    const u32 *var_allele_off; // [n_vars + 1]
};

__device__ __forceinline__ u32 site_u64_len(u64 m)
{
    u32 nd = 1;
    while (m >= 10u) {
        m /= 10u;
        ++nd;
    }
    return nd;
}
__device__ __forceinline__ void site_put_u64(const FmtWindow &w, u64 pos, u64 m)
{
    u64 at = pos + site_u64_len(m);
    do {
        w.put(--at, (char)('0' + (u32)(m % 10u)));
        m /= 10u;
    } while (m);
}
template <bool PUT>
__device__ __forceinline__ u64 site_put_str(const FmtWindow &w, u64 pos, const char *s, u32 n, bool writer)
{
    if (PUT && writer)
        for (u32 i = 0; i < n; ++i) w.put(pos + i, s[i]);
    return pos + n;
}

// AF of `ac` copies among `an`: the digits behind "0." (their trailing zeros gone) in *frac, how many in the result; 0: the one byte *lone
__device__ __forceinline__ u32 site_af_digits(u32 ac, u64 an, u32 *frac, char *lone)
{
    if (an == 0) {
        *lone = '.';
        return 0;
    }
    u32 q = (u32)((2ull * ac * 1000000ull + an) / (2ull * an));
    if (q == 0u || q >= 1000000u) {
        *lone = q ? '1' : '0';
        return 0;
    }
    u32 nd = 6;
    while (q % 10u == 0u) {
        q /= 10u;
        --nd;
    }
    *frac = q;
    return nd;
}

// The list behind AC= (AF false) or AF= (AF true): the record's ALT slots 64 at a time, every lane its item -- a comma in front of
// all but the first -- at the offset a wave prefix sum gives it.  Returns the position behind the list.
template <bool PUT, bool AF>
__device__ __forceinline__ u64 site_info_list(const InfoArgs &a, const FmtWindow &w, u32 a0, u32 A, u64 an, u32 lane, u64 pos)
{
    for (u32 base = 1; base < A; base += 64) {
        const u32 k = base + lane;
        const bool have = k < A;
        const u32 val = have ? a.ac[a0 + k] : 0u;
        u32 frac = 0, nd = 0, len = 0;
        char lone = 0;
        if (have) {
            if (AF) {
                nd = site_af_digits(val, an, &frac, &lone);
                len = nd ? 2 + nd : 1;
            } else
                len = site_u64_len(val);
            len += k > 1;
        }
        u32 incl = len;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 up = (u32)__shfl_up((int)incl, d, 64);
            if (lane >= (u32)d) incl += up;
        }
        if (PUT && have) {
            u64 at = pos + (incl - len);
            if (k > 1) w.put(at++, ',');
            if (!AF) site_put_u64(w, at, val);
            else if (!nd) w.put(at, lone);
            else {
                w.put(at, '0');
                w.put(at + 1, '.');
                for (u32 i = nd; i; --i) { // (zero-padded to nd digits)
                    w.put(at + 1 + i, (char)('0' + frac % 10u));
                    frac /= 10u;
                }
            }
        }
        pos += (u32)__shfl((int)incl, 63, 64);
    }
    return pos;
}

// row v from `pos` on, by one wave; returns the position behind it (PUT false: nothing is written, the length pass)
template <bool PUT>
__device__ __forceinline__ u64 site_info_row(const InfoArgs &a, const FmtWindow &w, u64 v, u32 lane, u64 pos)
{
    const u32 a0 = a.var_allele_off[v], A = a.var_allele_off[v + 1] - a0;
    unsigned long long an = 0;
    for (u32 k = lane; k < A; k += 64) an += a.ac[a0 + k];
    for (int d = 32; d; d >>= 1) an += (unsigned long long)__shfl_xor((long long)an, d, 64);
    const bool first = lane == 0;
    if (A > 1) {
        pos = site_put_str<PUT>(w, pos, "AC=", 3, first);
        pos = site_info_list<PUT, false>(a, w, a0, A, an, lane, pos);
        pos = site_put_str<PUT>(w, pos, ";AN=", 4, first);
    } else
        pos = site_put_str<PUT>(w, pos, "AN=", 3, first);
    if (PUT && first) site_put_u64(w, pos, an);
    pos += site_u64_len(an);
    if (A > 1) {
        pos = site_put_str<PUT>(w, pos, ";AF=", 4, first);
        pos = site_info_list<PUT, true>(a, w, a0, A, an, lane, pos);
    }
    pos = site_put_str<PUT>(w, pos, ";NS=", 4, first);
    const u32 s = a.ns[v];
    if (PUT && first) site_put_u64(w, pos, s);
    return pos + site_u64_len(s);
}

// meta[1] is raised when a row does not fit 32 bits, as by fmt_len_kernel
__global__ void __launch_bounds__(FMT_TPB) info_len_kernel(InfoArgs a, u32 *__restrict__ len, unsigned long long *meta)
{
    const u32 lane = threadIdx.x & 63;
    const u64 v = (u64)blockIdx.x * (FMT_TPB / 64) + (threadIdx.x >> 6);
    if (v >= a.n_vars) return; // (wave-uniform)
    const u64 bytes = site_info_row<false>(a, FmtWindow{nullptr, 0, 0}, v, lane, 0);
    if (lane == 0) {
        if (bytes > 0xFFFFFFFFull) atomicOr(meta + 1, 1ull);
        len[v] = (u32)bytes;
    }
}

struct InfoRows {
    InfoArgs a;
    __device__ __forceinline__ void put(const FmtWindow &w, u64 v, u32 lane, u64 r0, u64) const { site_info_row<true>(a, w, v, lane, r0); }
};

__global__ void __launch_bounds__(FMT_TPB) info_write_kernel(InfoArgs a, const unsigned long long *__restrict__ row_off, char *text, u64 text_cap)
{
    __shared__ __attribute__((aligned(16))) char sh[FMT_WINDOW];
    fmt_write_tile(InfoRows{a}, sh, a.n_vars, row_off, text, text_cap);
}

} // namespace
