// cohort_prior_kernels.h -- allele priors re-estimated from the planes of a batch, then every cell genotyped under them
// Part of the malva_hip translation unit: included by malva_hip.hip inside its anonymous namespace, after geno_dev.h.
// The definition is in include/malva_hip.h (mg_genotype_cohort) and DESIGN.md section 10; there is no reference call behind the
// estimate, the per-cell part is genotype_one (var_block.hpp:224-330, 366-394).
//
// Shape.  Lanes are planes: a record owns a segment of W lanes, W the smallest power of two >= n_planes, so a wave holds 64 / W
// records and a workgroup of four waves 256 / W.  A workgroup owns a run of consecutive records -- max(256 / W, 16) of them, so that
// a plane's row of the run is at least a cache line of biallelic records -- and first brings the run's slots of every plane into LDS
// with threads along the slots (coalesced per plane row); the lanes then read their record's coverages from there.  A run whose
// slots do not fit (a record with hundreds of alleles in it) reads global memory instead.
//   per lane, once:        the prior-free part of each genotype's log value (A == 2: two or three doubles in registers)
//   per iteration:         A == 2: the record's 2 or 3 log priors, one per lane of the segment in ONE logf_ref pass, handed round by
//                          shuffle; an exp_ref per genotype, the division, the expected ALT copies
//                          A 3..8: gt_value per genotype, twice (sum, then posteriors), copies in LDS
//                          the tree sum of the definition as an xor butterfly inside the segment (lane i < s adds lane i + s, which is
//                          lane i ^ s: the lowest lane ends with x[0] of the tree), broadcast from the lowest lane
//                          the update, by every lane of the segment alike (same operands, same operations)
//   at the end:            genotype_one per cell under f_T, its GT / GQ / status into LDS; the workgroup then writes the run's calls with
//                          threads along the records (lanes are planes: stored directly, every lane of a store would hit its own line)
// No lane leaves before the last cross-lane operation: idle lanes, finished segments and records that are not re-estimated carry
// +0.0 through the exchange.  No floating-point atomic anywhere.
// cohort_prior_wide_kernel (below): the estimate alone for any number of planes, the sum over planes continued across chunks of 64.
#pragma once

constexpr int PRIOR_TPB = 256;
constexpr u32 PRIOR_COV_CAP = 2560; // dwords of LDS for a run's coverages (sixteen biallelic records of 64 planes take 2112)
constexpr u32 PRIOR_MIN_RUN = 16;   // records per workgroup at the least
static_assert(MG_PRIOR_MAX_ALLELES == 8, "s_f, s_e and the fixed loops below are laid out for eight alleles");

struct PriorArgs {
    u64 n_vars;
    u32 n_planes, seg_log2, run, iters;
    double weight;
    const u32 *cov;   // [n_planes][slots]
    const float *freq; // [slots]
    const u32 *vao;   // [n_vars + 1]
    float *freq_out;  // [slots]
    u32 *n_inf;       // [n_vars]
    i32 *gt1, *gt2, *gq; // [n_planes][n_vars]
    u8 *status;
    double *probs;    // [n_planes][var_gt_off[n_vars]] or nullptr
    const u64 *var_gt_off;
};

// the prior-free part of gt_value (geno_dev.h), the same operations in the same order
__device__ __forceinline__ double prior_post_hom(u32 truth, u32 total, int A, const GenoParams &p)
{
    const u32 error = total - truth;
    const float t1 = (float)truth * p.c_hom;
    const float t2 = (float)error * c_err1(A, p);
    return log_binomial((int)(truth + error), (int)truth, p) + (double)t1 + (double)t2;
}
__device__ __forceinline__ double prior_post_het(u32 t1c, u32 t2c, u32 total, int A, const GenoParams &p)
{
    const u32 error = total - t1c - t2c;
    const float t1 = (float)t1c * p.c_het;
    const float t2 = (float)t2c * p.c_het;
    double log_post = log_binomial((int)(t1c + t2c + error), (int)(t1c + t2c), p) + log_binomial((int)(t1c + t2c), (int)t1c, p) + (double)t1 + (double)t2;
    if (A > 2) {
        const float t3 = (float)error * c_err2(A, p);
        log_post += (double)t3;
    }
    return log_post;
}
__device__ __forceinline__ double prior_value(double log_prior, double log_post)
{
    const double lp = log_prior + log_post;
    return isinf(lp) ? 0.0 : exp_ref(lp);
}
// f[0] from the ALT values as the panel parser makes it (host/io.hpp: frequencies[0])
__device__ __forceinline__ float prior_ref_freq(double acc)
{
    const float r = (float)(1.0 - acc);
    return r < 0 ? 0.0f : r;
}

__global__ void __launch_bounds__(PRIOR_TPB) cohort_prior_kernel(PriorArgs a, GenoParams p)
{
    __shared__ u32 s_cov[PRIOR_COV_CAP];
    __shared__ float s_f[PRIOR_TPB * MG_PRIOR_MAX_ALLELES];  // [record of the run][allele]: the record's current frequencies
    __shared__ double s_e[MG_PRIOR_MAX_ALLELES * PRIOR_TPB]; // [allele][thread]: a lane's expected copies (A > 2)
    __shared__ i32 s_call[3][64 * (PRIOR_MIN_RUN + 1)]; // gt1 / gt2 / gq of the run, [plane][record] at an odd stride: written out along the records
    __shared__ u8 s_stat[64 * (PRIOR_MIN_RUN + 1)];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 W = 1u << a.seg_log2, plane = lane & (W - 1), seg_base = lane & ~(W - 1), R = 64u >> a.seg_log2;
    const u64 seg_mask = W == 64 ? ~0ull : ((1ull << W) - 1) << seg_base;
    const u64 slots = a.vao[a.n_vars];
    const u64 v0 = (u64)blockIdx.x * a.run, v1 = v0 + a.run < a.n_vars ? v0 + a.run : a.n_vars;
    const u32 a_lo = a.vao[v0], span = a.vao[v1] - a_lo, stride = span | 1; // (odd: the planes of a record fall on different banks)
    const bool use_lds = (u64)a.n_planes * stride <= PRIOR_COV_CAP;
    const u32 ostride = a.run | 1; // (n_planes * ostride <= W * (max(256 / W, 16) + 1) <= 64 * 17)
    if (use_lds)
        for (u32 idx = tid; idx < a.n_planes * span; idx += PRIOR_TPB) {
            const u32 pl = idx / span, j = idx - pl * span;
            s_cov[pl * stride + j] = a.cov[pl * slots + a_lo + j];
        }
    __syncthreads();
    const bool mine = plane < a.n_planes; // this lane has a cell
    const int hap = p.haploid;
    const u32 ploidy = hap ? 1u : 2u;
    const int G2 = hap ? 2 : 3; // genotypes of a biallelic record
    for (u32 k = 0; k < a.run; k += 4 * R) {
        const u32 rec = k + wave * R + (lane >> a.seg_log2);
        const u64 v = v0 + rec;
        const bool seg_ok = v < v1;
        u32 a0 = 0;
        int A = 0;
        if (seg_ok) {
            a0 = a.vao[v];
            A = (int)(a.vao[v + 1] - a0);
        }
        const bool elig = seg_ok && A >= 2 && A <= MG_PRIOR_MAX_ALLELES && a.iters > 0; // the record is re-estimated (the whole segment agrees)
        const u32 row = mine ? plane : 0, rel = seg_ok ? a0 - a_lo : 0; // (a lane without a cell never reads through covp)
        const u32 *covp = use_lds ? &s_cov[row * stride + rel] : a.cov + row * slots + a_lo + rel;
        float *fseg = &s_f[rec * MG_PRIOR_MAX_ALLELES];
        const bool two = elig && A == 2;
        // the cell's status from its coverages, and what does not depend on the prior
        bool normal = false;
        u32 total = 0, c0 = 0, c1 = 0;
        float f0r = 1.f, f1r = 1.f; // A == 2: the record's frequencies
        double post0 = 0.0, post1 = 0.0, post2 = 0.0;
        if (elig) {
            for (int al = 0; al < A; ++al) fseg[al] = a.freq[a0 + al];
            if (two) {
                f0r = fseg[0];
                f1r = fseg[1];
            }
        }
        if (elig && mine) {
            bool over = false;
            int isum = 0;
            for (int al = 0; al < A; ++al) {
                over |= (int)covp[al] > p.max_cov;
                isum += (int)covp[al];
            }
            total = (u32)isum;
            normal = !over && total != 0;
            if (two && normal) {
                c0 = covp[0];
                c1 = covp[1];
                post0 = prior_post_hom(c0, total, 2, p);
                if (hap) post1 = prior_post_hom(c1, total, 2, p);
                else {
                    post1 = prior_post_het(c0, c1, total, 2, p);
                    post2 = prior_post_hom(c1, total, 2, p);
                }
            }
        }
        int amax = MG_PRIOR_MAX_ALLELES; // the largest A among the wave's re-estimated records
        while (amax > 2 && !__any(elig && A >= amax)) --amax;
        bool live = elig; // the segment still iterates
        u32 n_last = 0;
        for (u32 t = 0; t < a.iters && __any(live); ++t) {
            // A == 2: the log priors, genotype g by lane g of the segment (W < G2: in several passes)
            double L0 = 0.0, L1 = 0.0, L2 = 0.0;
            if (__any(live && two))
                for (u32 base = 0; base < (u32)G2; base += W) {
                    const u32 g = base + plane;
                    const bool het = !hap && g == 1;
                    const float x = het ? 2 * f0r * f1r : (g == 0 ? f0r : f1r);
                    const float l = logf_ref(x);
                    const double m = het ? (double)l : (double)(2 * l);
                    if (base <= 0 && 0 < base + W) L0 = __shfl(m, (int)(seg_base + 0 - base));
                    if (base <= 1 && 1 < base + W) L1 = __shfl(m, (int)(seg_base + 1 - base));
                    if (G2 > 2 && base <= 2 && 2 < base + W) L2 = __shfl(m, (int)(seg_base + 2 - base));
                }
            // posteriors and expected copies of this lane's cell
            bool counts = false;
            double e1 = 0.0;
            if (live && mine && normal) {
                if (two) {
                    const double w0 = prior_value(L0, post0), w1 = prior_value(L1, post1);
                    if (hap) {
                        const double sum = 0.0 + w0 + w1;
                        counts = isfinite(sum) && sum > 0;
                        if (counts) e1 = 0.0 + w1 / sum;
                    } else {
                        const double w2 = prior_value(L2, post2);
                        const double sum = 0.0 + w0 + w1 + w2;
                        counts = isfinite(sum) && sum > 0;
                        if (counts) {
                            e1 = 0.0 + w1 / sum;
                            e1 = e1 + 2.0 * (w2 / sum);
                        }
                    }
                } else {
                    double sum = 0.0;
                    for (int g1 = 0; g1 < A; ++g1)
                        for (int g2 = hap ? -1 : g1; g2 < (hap ? 0 : A); ++g2) sum += gt_value(covp, fseg, A, total, g1, g2, p);
                    counts = isfinite(sum) && sum > 0;
                    if (counts) {
                        for (int al = 0; al < A; ++al) s_e[al * PRIOR_TPB + tid] = 0.0;
                        for (int g1 = 0; g1 < A; ++g1)
                            for (int g2 = hap ? -1 : g1; g2 < (hap ? 0 : A); ++g2) {
                                const double q = gt_value(covp, fseg, A, total, g1, g2, p) / sum;
                                if (hap) s_e[g1 * PRIOR_TPB + tid] += q;
                                else if (g1 == g2) s_e[g1 * PRIOR_TPB + tid] += 2.0 * q;
                                else {
                                    s_e[g1 * PRIOR_TPB + tid] += q;
                                    s_e[g2 * PRIOR_TPB + tid] += q;
                                }
                            }
                    }
                }
            }
            const u32 n = (u32)__popcll(__ballot(counts) & seg_mask);
            const bool upd = live && n > 0;
            bool changed = false;
            double acc = 0.0;
            acc += 0.f;
            for (int al = 1; al < amax; ++al) {
                double x = 0.0;
                if (counts && al < A) x = two ? e1 : s_e[al * PRIOR_TPB + tid];
                for (u32 s = W >> 1; s; s >>= 1) x = x + __shfl_xor(x, (int)s);
                const double c = __shfl(x, (int)seg_base);
                if (upd && al < A) {
                    const double f0a = (double)a.freq[a0 + al];
                    const double wf = a.weight * f0a;
                    const double num = c + wf;
                    const double den = (double)(ploidy * n) + a.weight;
                    const float fn = (float)(num / den);
                    const float old = two ? f1r : fseg[al];
                    changed |= __float_as_uint(fn) != __float_as_uint(old);
                    if (two) f1r = fn;
                    else fseg[al] = fn;
                    acc += fn;
                }
            }
            if (live) {
                n_last = n;
                if (upd) {
                    const float fr = prior_ref_freq(acc);
                    const float old = two ? f0r : fseg[0];
                    changed |= __float_as_uint(fr) != __float_as_uint(old);
                    if (two) f0r = fr;
                    else fseg[0] = fr;
                }
                live = changed; // n == 0 or a repeat: every later iteration would give the same again
            }
        }
        if (two) {
            fseg[0] = f0r;
            fseg[1] = f1r;
        }
        // the cells under the final frequencies; the record's frequencies and n by the segment's lowest lane
        const float *fp = elig ? fseg : a.freq + a0;
        if (seg_ok && mine) {
            const u32 cell = plane * ostride + rec;
            genotype_one(covp, fp, A, p, &s_call[0][cell], &s_call[1][cell], &s_call[2][cell], &s_stat[cell],
                         a.probs ? a.probs + plane * a.var_gt_off[a.n_vars] + a.var_gt_off[v] : nullptr);
        }
        if (seg_ok && plane == 0) {
            for (int al = 0; al < A; ++al) a.freq_out[a0 + al] = fp[al];
            a.n_inf[v] = n_last;
        }
    }
    // the run's calls, threads along the records: a plane's row of the run is one contiguous piece of every output array
    __syncthreads();
    const u32 run_len = (u32)(v1 - v0);
    for (u32 idx = tid; idx < a.n_planes * run_len; idx += PRIOR_TPB) {
        const u32 pl = idx / run_len, j = idx - pl * run_len;
        const u64 cell = (u64)pl * a.n_vars + v0 + j;
        a.gt1[cell] = s_call[0][pl * ostride + j];
        a.gt2[cell] = s_call[1][pl * ostride + j];
        a.gq[cell] = s_call[2][pl * ostride + j];
        a.status[cell] = s_stat[pl * ostride + j];
    }
}

// ---- the estimate alone, for any number of planes (mg_estimate_priors) -------------------------------------------------------------------
// The same estimate with the sum over planes extended past one wave: planes are cut into chunks of 64 in the order given, a chunk's
// tree C_j is the butterfly above, and the record's c[a] = C_0[a] + C_1[a] + .. in chunk order, each add rounded on its own
// (include/malva_hip.h, mg_estimate_priors).  No calls: the cells are genotyped afterwards by mg_genotype_cohort(iters = 0, freq = f_T).
//
// Shape.  Up to 64 planes: the segment widths, the run and the LDS staging of cohort_prior_kernel, one chunk, the run staged once.
// Beyond: every chunk runs at segment width 64 (e >= +0.0 and x + (+0.0) = x for such x, so padding a short chunk to 64 lanes gives
// the C_j of its own power of two), a wave holds one record at a time and a workgroup a run of 16.  Records are independent, so the
// whole EM of a record stays inside the workgroup that owns its run:
//   iteration (outer)      left by the whole workgroup once none of the run's records still iterates (__syncthreads_or)
//     chunk (inner)        P > 64: the workgroup stages the chunk's rows of the run into s_cov, between two barriers
//       records of the run, 256 / W at a time: status and the prior-free parts from the coverages (recomputed: they cannot stay in
//                          registers across chunks), the copies, the butterfly, and c = c + C_j by every lane of the segment alike;
//                          behind the last chunk the update
// What a record carries from chunk to chunk and from iteration to iteration lies in LDS, written by every lane of its segment with
// the same value: f (s_f), the running c and n (s_c, s_n: only P > 64 needs them, where the run is 16), live and the last n.
// Trip counts: iterations and chunks are workgroup-uniform, the records' steps and the alleles' (amax) wave-uniform; a finished
// record, an idle lane and a plane that does not count carry +0.0 through the exchange, no lane leaves early.  One launch, no global
// intermediates, no floating-point atomic.
constexpr u32 PRIOR_WIDE_RUN = 16; // records per workgroup beyond 64 planes (s_c, s_n)

struct PriorWideArgs {
    u64 n_vars;
    u32 n_planes, seg_log2, run, iters, n_chunks;
    double weight;
    const u32 *cov;    // [n_planes][slots]
    const float *freq; // [slots]
    const u32 *vao;    // [n_vars + 1]
    float *freq_out;   // [slots]
    u32 *n_inf;        // [n_vars]
};

__global__ void __launch_bounds__(PRIOR_TPB) cohort_prior_wide_kernel(PriorWideArgs a, GenoParams p)
{
    __shared__ u32 s_cov[PRIOR_COV_CAP];
    __shared__ float s_f[PRIOR_TPB * MG_PRIOR_MAX_ALLELES];  // [record of the run][allele]: the record's current frequencies
    __shared__ double s_e[MG_PRIOR_MAX_ALLELES * PRIOR_TPB]; // [allele][thread]: a lane's expected copies (A > 2)
    __shared__ double s_c[PRIOR_WIDE_RUN * MG_PRIOR_MAX_ALLELES]; // [record of the run][allele]: C_0 + .. + C_j so far (P > 64)
    __shared__ u32 s_n[PRIOR_WIDE_RUN];                      // the planes that count so far in this iteration (P > 64)
    __shared__ u32 s_vao[PRIOR_TPB + 1];                     // the run's allele offsets
    __shared__ u32 s_nlast[PRIOR_TPB];                       // n of the last iteration the record ran
    __shared__ u8 s_live[PRIOR_TPB];                         // the record still iterates
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 W = 1u << a.seg_log2, plane = lane & (W - 1), seg_base = lane & ~(W - 1), R = 64u >> a.seg_log2;
    const u64 seg_mask = W == 64 ? ~0ull : ((1ull << W) - 1) << seg_base;
    const u64 slots = a.vao[a.n_vars];
    const u64 v0 = (u64)blockIdx.x * a.run, v1 = v0 + a.run < a.n_vars ? v0 + a.run : a.n_vars;
    const u32 run_len = (u32)(v1 - v0);
    const u32 a_lo = a.vao[v0], span = a.vao[v1] - a_lo, stride = span | 1; // (odd: the planes of a record fall on different banks)
    const u32 rows_max = a.n_planes < 64 ? a.n_planes : 64;                 // the planes of a full chunk
    const bool use_lds = (u64)rows_max * stride <= PRIOR_COV_CAP;
    const bool wide = a.n_chunks > 1;
    for (u32 r = tid; r <= run_len; r += PRIOR_TPB) s_vao[r] = a.vao[v0 + r];
    __syncthreads();
    if (tid < run_len) { // (run <= PRIOR_TPB)
        const u32 a0 = s_vao[tid];
        const int A = (int)(s_vao[tid + 1] - a0);
        const bool elig = A >= 2 && A <= MG_PRIOR_MAX_ALLELES && a.iters > 0;
        if (elig)
            for (int al = 0; al < A; ++al) s_f[tid * MG_PRIOR_MAX_ALLELES + al] = a.freq[a0 + al];
        s_live[tid] = elig;
        s_nlast[tid] = 0;
    }
    if (!wide && use_lds)
        for (u32 idx = tid; idx < a.n_planes * span; idx += PRIOR_TPB) {
            const u32 pl = idx / span, j = idx - pl * span;
            s_cov[pl * stride + j] = a.cov[pl * slots + a_lo + j];
        }
    const int hap = p.haploid;
    const u32 ploidy = hap ? 1u : 2u;
    const int G2 = hap ? 2 : 3; // genotypes of a biallelic record
    for (u32 t = 0; t < a.iters; ++t) {
        __syncthreads(); // behind the set-up and the last iteration's updates: s_live is read across waves
        if (!__syncthreads_or(tid < run_len && s_live[tid])) break;
        for (u32 ch = 0; ch < a.n_chunks; ++ch) {
            const u32 p_lo = ch * 64, rows = a.n_planes - p_lo < 64 ? a.n_planes - p_lo : 64;
            if (wide) {
                __syncthreads(); // the chunk before has been read
                if (use_lds)
                    for (u32 idx = tid; idx < rows * span; idx += PRIOR_TPB) {
                        const u32 pl = idx / span, j = idx - pl * span;
                        s_cov[pl * stride + j] = a.cov[(u64)(p_lo + pl) * slots + a_lo + j];
                    }
                __syncthreads();
            }
            const bool mine = plane < rows; // this lane has a cell in this chunk
            const bool last = ch + 1 == a.n_chunks;
            for (u32 k = 0; k < a.run; k += 4 * R) {
                const u32 rec = k + wave * R + (lane >> a.seg_log2);
                const bool seg_ok = rec < run_len;
                u32 a0 = 0;
                int A = 0;
                if (seg_ok) {
                    a0 = s_vao[rec];
                    A = (int)(s_vao[rec + 1] - a0);
                }
                const bool live = seg_ok && A >= 2 && A <= MG_PRIOR_MAX_ALLELES && s_live[rec]; // (the whole segment agrees)
                const u32 row = mine ? plane : 0, rel = seg_ok ? a0 - a_lo : 0; // (a lane without a cell never reads through covp)
                const u32 *covp = use_lds ? &s_cov[row * stride + rel] : a.cov + (u64)(p_lo + row) * slots + a_lo + rel;
                float *fseg = &s_f[rec * MG_PRIOR_MAX_ALLELES];
                const bool two = live && A == 2;
                // the cell's status from its coverages, and what does not depend on the prior
                bool normal = false;
                u32 total = 0;
                float f0r = 1.f, f1r = 1.f; // A == 2: the record's frequencies
                double post0 = 0.0, post1 = 0.0, post2 = 0.0;
                if (two) {
                    f0r = fseg[0];
                    f1r = fseg[1];
                }
                if (live && mine) {
                    bool over = false;
                    int isum = 0;
                    for (int al = 0; al < A; ++al) {
                        over |= (int)covp[al] > p.max_cov;
                        isum += (int)covp[al];
                    }
                    total = (u32)isum;
                    normal = !over && total != 0;
                    if (two && normal) {
                        const u32 c0 = covp[0], c1 = covp[1];
                        post0 = prior_post_hom(c0, total, 2, p);
                        if (hap) post1 = prior_post_hom(c1, total, 2, p);
                        else {
                            post1 = prior_post_het(c0, c1, total, 2, p);
                            post2 = prior_post_hom(c1, total, 2, p);
                        }
                    }
                }
                int amax = MG_PRIOR_MAX_ALLELES; // the largest A among the wave's records that still iterate
                while (amax > 2 && !__any(live && A >= amax)) --amax;
                // A == 2: the log priors, genotype g by lane g of the segment (W < G2: in several passes)
                double L0 = 0.0, L1 = 0.0, L2 = 0.0;
                if (__any(two))
                    for (u32 base = 0; base < (u32)G2; base += W) {
                        const u32 g = base + plane;
                        const bool het = !hap && g == 1;
                        const float x = het ? 2 * f0r * f1r : (g == 0 ? f0r : f1r);
                        const float l = logf_ref(x);
                        const double m = het ? (double)l : (double)(2 * l);
                        if (base <= 0 && 0 < base + W) L0 = __shfl(m, (int)(seg_base + 0 - base));
                        if (base <= 1 && 1 < base + W) L1 = __shfl(m, (int)(seg_base + 1 - base));
                        if (G2 > 2 && base <= 2 && 2 < base + W) L2 = __shfl(m, (int)(seg_base + 2 - base));
                    }
                // posteriors and expected copies of this lane's cell
                bool counts = false;
                double e1 = 0.0;
                if (live && mine && normal) {
                    if (two) {
                        const double w0 = prior_value(L0, post0), w1 = prior_value(L1, post1);
                        if (hap) {
                            const double sum = 0.0 + w0 + w1;
                            counts = isfinite(sum) && sum > 0;
                            if (counts) e1 = 0.0 + w1 / sum;
                        } else {
                            const double w2 = prior_value(L2, post2);
                            const double sum = 0.0 + w0 + w1 + w2;
                            counts = isfinite(sum) && sum > 0;
                            if (counts) {
                                e1 = 0.0 + w1 / sum;
                                e1 = e1 + 2.0 * (w2 / sum);
                            }
                        }
                    } else {
                        double sum = 0.0;
                        for (int g1 = 0; g1 < A; ++g1)
                            for (int g2 = hap ? -1 : g1; g2 < (hap ? 0 : A); ++g2) sum += gt_value(covp, fseg, A, total, g1, g2, p);
                        counts = isfinite(sum) && sum > 0;
                        if (counts) {
                            for (int al = 0; al < A; ++al) s_e[al * PRIOR_TPB + tid] = 0.0;
                            for (int g1 = 0; g1 < A; ++g1)
                                for (int g2 = hap ? -1 : g1; g2 < (hap ? 0 : A); ++g2) {
                                    const double q = gt_value(covp, fseg, A, total, g1, g2, p) / sum;
                                    if (hap) s_e[g1 * PRIOR_TPB + tid] += q;
                                    else if (g1 == g2) s_e[g1 * PRIOR_TPB + tid] += 2.0 * q;
                                    else {
                                        s_e[g1 * PRIOR_TPB + tid] += q;
                                        s_e[g2 * PRIOR_TPB + tid] += q;
                                    }
                                }
                        }
                    }
                }
                // n and c over the chunks so far (rec < PRIOR_WIDE_RUN wherever there is more than one chunk)
                u32 n = (u32)__popcll(__ballot(counts) & seg_mask);
                if (ch > 0) n += s_n[rec];
                if (wide && !last && live) s_n[rec] = n;
                const bool upd = live && last && n > 0;
                bool changed = false;
                double acc = 0.0;
                acc += 0.f;
                for (int al = 1; al < amax; ++al) {
                    double x = 0.0;
                    if (counts && al < A) x = two ? e1 : s_e[al * PRIOR_TPB + tid];
                    for (u32 s = W >> 1; s; s >>= 1) x = x + __shfl_xor(x, (int)s);
                    double c = __shfl(x, (int)seg_base);
                    if (live && al < A) {
                        if (ch > 0) c = s_c[rec * MG_PRIOR_MAX_ALLELES + al] + c;
                        if (wide && !last) s_c[rec * MG_PRIOR_MAX_ALLELES + al] = c;
                    }
                    if (upd && al < A) {
                        const double f0a = (double)a.freq[a0 + al];
                        const double wf = a.weight * f0a;
                        const double num = c + wf;
                        const double den = (double)(ploidy * n) + a.weight;
                        const float fn = (float)(num / den);
                        changed |= __float_as_uint(fn) != __float_as_uint(fseg[al]);
                        fseg[al] = fn;
                        acc += fn;
                    }
                }
                if (live && last) {
                    s_nlast[rec] = n;
                    if (upd) {
                        const float fr = prior_ref_freq(acc);
                        changed |= __float_as_uint(fr) != __float_as_uint(fseg[0]);
                        fseg[0] = fr;
                    }
                    s_live[rec] = changed; // n == 0 or a repeat: every later iteration would give the same again
                }
            }
        }
    }
    // the records' frequencies and n, threads along the records
    __syncthreads();
    if (tid < run_len) {
        const u32 a0 = s_vao[tid], A = s_vao[tid + 1] - a0;
        const bool elig = A >= 2 && A <= MG_PRIOR_MAX_ALLELES && a.iters > 0;
        for (u32 al = 0; al < A; ++al) a.freq_out[a0 + al] = elig ? s_f[tid * MG_PRIOR_MAX_ALLELES + al] : a.freq[a0 + al];
        a.n_inf[v0 + tid] = s_nlast[tid];
    }
}
