// The per-sample table of a multi-sample call set: for every plane (sample) the sums of its cells along the records -- how many are
// called, masked, heterozygous, of which kind their alleles are, the GQ sum and histogram, the coverage, the genotyper's status codes:
// MG_SAMPLE_SLOTS 64-bit counters per plane (include/malva_hip.h, MG_SS_*).  mg_site_counts sums the cell matrix along the samples, this
// along the records.  The reference -- one individual per run -- has nothing like it.
//
// Ownership (mg_sample_counts_device): sample_count_kernel runs on a grid of (runs of records, planes).  A workgroup of SAMPLE_TPB
// threads owns one plane and one run; its waves take 64 consecutive records each and step through the run SAMPLE_TPB records at a
// time.  The arrays are plane-major, so a wave's loads of gt1 / gt2 / gq / status are coalesced; the ragged coverages of a lane's record,
// cov[p][a0 .. a0 + A), lie behind its left neighbour's, so the lanes' walks are neighbours too.  A slot that counts cells is
// popcount(ballot(predicate)) added to a wave-uniform 32-bit accumulator; GQ_SUM and COV_SUM are 64-bit per-lane sums from the first
// add (a coverage is any u32), reduced across the wave once behind the run.  Lane 0 of every wave puts the wave's sums into its own
// row of an LDS table; behind one barrier thread t < MG_SS_COUNTED adds the rows' column t and, unless it is zero, issues one 64-bit
// atomic add to counts[p][t]: one atomic wave-instruction per workgroup, not per record.
//
// Why no race: the LDS rows are written by one lane each and read behind the barrier; the workgroups of a plane's runs meet in
// counts[p] through atomic adds alone, and the sums are integers (GQ_SUM in two's complement), so the result does not depend on the
// order -- it is the same in every run and for every cut of the records into calls.  `accumulate == 0` is a hipMemsetAsync of all
// n_planes * MG_SAMPLE_SLOTS entries in front of the kernel, the reserved slots included; with `accumulate` the kernel only adds, and
// adds nothing to a slot whose input array is absent.  Nothing else of `counts` is touched: a plane is blockIdx.y < n_planes.
//
// Overflow: a 32-bit accumulator grows by at most 128 per step (a cell gives at most 2, to a class slot: a 1/2 cell of two
// transitions) and a wave takes run / SAMPLE_TPB steps with run <= SAMPLE_MAX_RUN = 2^20 (sample_count_plan): below 2^19.  The
// 64-bit sums: n_vars < 2^32 per call and a record's coverages below 2^32 each wrap only behind 2^64 / 2^32 = 2^32 slots of one
// plane in one call -- the caller's table is 64-bit and wraps there as well, by definition.
#pragma once
#include "call_text_kernels.h"
#include "count_plan.h" // SAMPLE_TPB, SAMPLE_MAX_RUN, sample_count_plan (plain C++: malva_hip.hip includes it first, outside every namespace)

namespace {
using namespace mg;

static_assert(MG_SAMPLE_SLOTS == 32 && MG_SS_COUNTED == 29 && MG_SS_GQ_0 + 10 == MG_SS_COUNTED, "the slot table of include/malva_hip.h");

struct SampleArgs {
    u64 n_vars, run;           // records; records per workgroup (a multiple of SAMPLE_TPB)
    int haploid;
    const i32 *gt1, *gt2, *gq; // [n_planes][n_vars]
    int use_mask;
    i32 min_gq;
    const u8 *status;          // [n_planes][n_vars] or nullptr
    const u32 *cov;            // [n_planes][slots], slots = var_allele_off[n_vars] (read here: the device form has no host copy), or nullptr
    const u32 *var_allele_off; // [n_vars + 1]
    const u8 *allele_class;    // [slots] or nullptr
};

__device__ __forceinline__ u32 sample_votes(bool pred) { return (u32)__popcll(__ballot(pred)); }

// grid: (ceil(n_vars / run), n_planes)
__global__ void __launch_bounds__(SAMPLE_TPB) sample_count_kernel(SampleArgs a, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long part[SAMPLE_TPB / 64][MG_SAMPLE_SLOTS];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = blockIdx.y;
    const u64 v_begin = (u64)blockIdx.x * a.run, v_end = v_begin + a.run < a.n_vars ? v_begin + a.run : a.n_vars;
    u32 cnt[MG_SS_COUNTED]; // wave-uniform (below 2^19: the head of this file); [MG_SS_GQ_SUM] and [MG_SS_COV_SUM] stay 0
#pragma unroll
    for (u32 k = 0; k < MG_SS_COUNTED; ++k) cnt[k] = 0;
    long long gq_sum = 0;
    unsigned long long cov_sum = 0;
    const u64 slots = a.cov ? a.var_allele_off[a.n_vars] : 0; // (uniform)
    for (u64 v0 = v_begin + (u64)wave * 64; v0 < v_end; v0 += SAMPLE_TPB) { // (wave-uniform)
        const u64 v = v0 + lane;
        const bool live = v < v_end;
        u32 g1 = 0, g2 = 0, a0 = 0, A = 0, st = ~0u;
        i32 q = 0;
        if (live) {
            const u64 i = (u64)p * a.n_vars + v;
            g1 = (u32)a.gt1[i];
            g2 = a.haploid ? g1 : (u32)a.gt2[i];
            q = a.gq[i];
            a0 = a.var_allele_off[v];
            A = a.var_allele_off[v + 1] - a0;
            if (a.status) st = a.status[i];
        }
        const bool masked = live && a.use_mask && q < a.min_gq;
        const bool bad = live && !masked && (g1 >= A || g2 >= A); // (unsigned: a negative index is beyond every A)
        const bool called = live && !masked && !bad;
        const bool het = called && g1 != g2;
        cnt[MG_SS_RECORDS] += sample_votes(live);
        cnt[MG_SS_MASKED] += sample_votes(masked);
        cnt[MG_SS_BAD] += sample_votes(bad);
        cnt[MG_SS_CALLED] += sample_votes(called);
        cnt[MG_SS_HOM_REF] += sample_votes(called && (g1 | g2) == 0u);
        cnt[MG_SS_HET] += sample_votes(het);
        cnt[MG_SS_HOM_ALT] += sample_votes(called && g1 != 0u && g1 == g2);
        cnt[MG_SS_HET_ALT] += sample_votes(het && g1 != 0u && g2 != 0u);
        if (a.allele_class) {
            // the distinct nonzero indexes of a called cell: gt1, and gt2 where it differs (haploid: g2 == g1)
            u32 c1 = 0, c2 = 0;
            if (called && g1 != 0u && g1 < A) c1 = a.allele_class[(u64)a0 + g1];
            if (het && g2 != 0u && g2 < A) c2 = a.allele_class[(u64)a0 + g2];
#pragma unroll
            for (u32 k = 1; k <= 5; ++k) cnt[MG_SS_TS + k - 1] += sample_votes(c1 == k) + sample_votes(c2 == k);
        }
        if (called) gq_sum += (long long)q;
        if (a.cov && live) {
            const u32 *row = a.cov + (u64)p * slots + a0;
            for (u32 s = 0; s < A; ++s) cov_sum += (unsigned long long)row[s];
        }
        if (a.status) {
#pragma unroll
            for (u32 k = 0; k < 4; ++k) cnt[MG_SS_ST_NORMAL + k] += sample_votes(st == k); // (a lane that is not live: ~0)
        }
        const u32 bin = live && !bad ? (u32)(q < 0 ? 0 : q > 99 ? 99 : q) / 10u : ~0u;
#pragma unroll
        for (u32 k = 0; k < 10; ++k) cnt[MG_SS_GQ_0 + k] += sample_votes(bin == k);
    }
    for (u32 off = 32; off; off >>= 1) {
        gq_sum += __shfl_down(gq_sum, off);
        cov_sum += __shfl_down(cov_sum, off);
    }
    if (lane == 0) {
#pragma unroll
        for (u32 k = 0; k < MG_SS_COUNTED; ++k) part[wave][k] = cnt[k];
        part[wave][MG_SS_GQ_SUM] = (unsigned long long)gq_sum;
        part[wave][MG_SS_COV_SUM] = cov_sum;
    }
    __syncthreads();
    if (threadIdx.x < MG_SS_COUNTED) {
        unsigned long long sum = 0;
#pragma unroll
        for (u32 w = 0; w < SAMPLE_TPB / 64; ++w) sum += part[w][threadIdx.x];
        if (sum) atomicAdd(counts + (u64)p * MG_SAMPLE_SLOTS + threadIdx.x, sum);
    }
}

} // namespace
