// Phred-scaled genotype likelihoods (the FORMAT field PL of the merged output) made from the coverages: mg_phred_likelihoods.
//
// What GP carries -- gt_value's exp(log_prior + log_post) -- has the allele-frequency prior folded in; PL is log_post alone, the part of
// gt_value that the genotype calls throw away, scaled and rounded the way bcftools writes it.  No frequencies are read.
//
// The values of a record are in VCF order: genotype j/k (j <= k) at index k (k + 1) / 2 + j of the record's slice, in haploid mode the
// allele.  (`probs` of the genotype calls is in the reference's order; the encoders copy PL and do not permute.)
//
// The cell (p, v).  A = the record's alleles, G = A in haploid mode, else A (A + 1) / 2.
//   1. If any (int)cov[a] > max_cov, all G values are MG_PL_MISSING: the over-covered cell the reference refuses to genotype.
//   2. If A == 1, the one value is 0 and nothing is computed (logf(e / (A - 1)) is infinite there).
//   3. If A == 0, nothing is written.
//   4. Otherwise, for every genotype g, lp_g is the log_post of gt_value (geno_dev.h: gt_log_post, its restatement) -- the host-made
//      ln table, log_binomial, every (float)count * constant product rounded to float before it joins the double sum, c_err2 only for
//      A > 2, no FMA contraction.  A cell whose total coverage is 0 falls out of this as all zeros: the honest likelihood of no data,
//      and not missing.
//   5. M is the largest finite lp_g.  If there is none, every value of the cell is missing.
//   6. For every g: a NaN or +inf lp_g gives a missing value.  Otherwise d = M - lp_g, x = d * K with K the double 0x1.15f2ced384f29p+2
//      (the double nearest to 10 / ln 10; the host's 10 / log(10) is one ulp below it), and PL = cap when x >= (double)cap, else
//      (int32_t)(x + 0.5); -inf therefore gives cap.  The subtract, the multiply and the add are each rounded on their own.
//
// Where it is bit-exact: with every record's total coverage below MG_LN_TABLE (65536) the result is bit-identical to a CPU restatement
// of the above (tests/pl_model.py).  At or above that total ln(n) is the device's log(double), as in mg_genotype_device, and the host
// form does not compute such a record again.
//
// Shape: one thread per cell, consecutive threads the consecutive records of one plane (blockIdx.y), so that cov at var_allele_off[v] and
// the output at var_gt_off[v] are read and written contiguously; no LDS; the biallelic diploid cell -- nearly every cell -- keeps its
// three values in registers.  No exponential and no division: the kernel is bound by its traffic, 4 A bytes in and 4 G bytes out per
// cell.  A record whose slice of var_gt_off is not G long is left alone (nothing is written outside a record's own slice).
#pragma once
#include "geno_dev.h"

namespace {
using namespace mg;

constexpr int PL_TPB = 256;
constexpr i32 PL_MISSING = INT32_MIN; // MG_PL_MISSING

struct PlArgs {
    u64 n_vars;
    const u32 *cov;            // [n_planes][var_allele_off[n_vars]]
    const u32 *var_allele_off; // [n_vars + 1]
    const u64 *var_gt_off;     // [n_vars + 1]
    i32 cap;                   // >= 1
    i32 *pl;                   // [n_planes][var_gt_off[n_vars]]
};

__device__ __forceinline__ bool pl_finite(double x) { return ((u64)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

// step 6 for one value
__device__ __forceinline__ i32 pl_value(double lp, double M, i32 cap)
{
    if (lp != lp || lp == INFINITY) return PL_MISSING;
    const double d = M - lp;
    const double x = d * 0x1.15f2ced384f29p+2;
    if (x >= (double)cap) return cap;
    return (i32)(x + 0.5);
}

__global__ void __launch_bounds__(PL_TPB) pl_kernel(PlArgs a, GenoParams p)
{
    const u64 v = (u64)blockIdx.x * PL_TPB + threadIdx.x;
    if (v >= a.n_vars) return;
    const u32 a0 = a.var_allele_off[v], A = a.var_allele_off[v + 1] - a0;
    const u64 g0 = a.var_gt_off[v], span = a.var_gt_off[v + 1] - g0;
    const u64 G = p.haploid ? (u64)A : (u64)A * (A + 1) / 2;
    if (A == 0 || span != G) return;
    const u32 *cov = a.cov + (u64)blockIdx.y * a.var_allele_off[a.n_vars] + a0;
    i32 *out = a.pl + (u64)blockIdx.y * a.var_gt_off[a.n_vars] + g0;
    if (A == 2 && !p.haploid) { // the biallelic diploid cell: 0/0, 0/1, 1/1 in registers
        const u32 c0 = cov[0], c1 = cov[1];
        const u32 c[2] = {c0, c1};
        i32 r0 = PL_MISSING, r1 = PL_MISSING, r2 = PL_MISSING;
        if ((int)c0 <= p.max_cov && (int)c1 <= p.max_cov) {
            const u32 total = (u32)((int)c0 + (int)c1);
            const double l00 = gt_log_post(c, 2, total, 0, 0, p), l01 = gt_log_post(c, 2, total, 0, 1, p), l11 = gt_log_post(c, 2, total, 1, 1, p);
            double M = -INFINITY;
            if (pl_finite(l00) && l00 > M) M = l00;
            if (pl_finite(l01) && l01 > M) M = l01;
            if (pl_finite(l11) && l11 > M) M = l11;
            if (pl_finite(M)) {
                r0 = pl_value(l00, M, a.cap);
                r1 = pl_value(l01, M, a.cap);
                r2 = pl_value(l11, M, a.cap);
            }
        }
        out[0] = r0;
        out[1] = r1;
        out[2] = r2;
        return;
    }
    bool over = false;
    int isum = 0;
    for (u32 s = 0; s < A; ++s) {
        over |= (int)cov[s] > p.max_cov;
        isum += (int)cov[s];
    }
    if (over) {
        for (u64 g = 0; g < G; ++g) out[g] = PL_MISSING;
        return;
    }
    if (A == 1) {
        out[0] = 0;
        return;
    }
    const u32 total = (u32)isum;
    // pass 1: the largest finite value; pass 2: the values again, scaled (the output holds no doubles, and nothing else is there to keep them)
    double M = -INFINITY;
    if (p.haploid) {
        for (u32 k = 0; k < A; ++k) {
            const double lp = gt_log_post(cov, (int)A, total, (int)k, -1, p);
            if (pl_finite(lp) && lp > M) M = lp;
        }
    } else {
        for (u32 k = 0; k < A; ++k)
            for (u32 j = 0; j <= k; ++j) {
                const double lp = gt_log_post(cov, (int)A, total, (int)j, (int)k, p);
                if (pl_finite(lp) && lp > M) M = lp;
            }
    }
    if (!pl_finite(M)) {
        for (u64 g = 0; g < G; ++g) out[g] = PL_MISSING;
        return;
    }
    if (p.haploid) {
        for (u32 k = 0; k < A; ++k) out[k] = pl_value(gt_log_post(cov, (int)A, total, (int)k, -1, p), M, a.cap);
    } else {
        u64 g = 0;
        for (u32 k = 0; k < A; ++k)
            for (u32 j = 0; j <= k; ++j, ++g) out[g] = pl_value(gt_log_post(cov, (int)A, total, (int)j, (int)k, p), M, a.cap);
    }
}

} // namespace
