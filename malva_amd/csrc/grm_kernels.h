// The genetic relationship matrix of a multi-sample call set: for every pair of samples the sum over the records of the product of their
// standardised dosages, in 16-bit fixed point, exact.  The reference -- one individual per run -- has nothing like it.  The definition is in
// include/malva_hip.h (mg_grm_step); tests/grm_model.py restates it.
//
// Weights (grm_weights_kernel): one thread per record, the lane along the records, so the loads of sites[group][dosage][record] are
// coalesced.  It popcounts the record's words over the groups (the bits at and beyond n_samples masked off), forms AN, AC and D in integers
// and q_d = rint((d AN - 2 AC) 1024 / sqrt((double)D)): one IEEE binary64 sqrt, one divide, one round-half-even -- the library is built
// without fast-math and with -ffp-contract=off, and both operations are spelled __dsqrt_rn / __ddiv_rn.  q[record] = {q0, q1, q2, enters},
// all 0 when the record does not enter.  A wave adds its entering records to *entered with one atomic.
//
// Expand (grm_expand_kernel): a thread takes four neighbouring records of one group and walks the group's 64 samples; per sample it
// stores one 32-bit word -- the four records' bytes -- to each of three images [sample][record], the record index contiguous:
//   L = ((q + 128) & 255) - 128,  H = (q - L) >> 8  (q = 256 H + L, both signed bytes),  C = 1,  q the weight of the cell's dosage;
// all three 0 where the cell does not contribute or the record does not enter.  Rows are padded to GRM_BLOCK samples and records to GRM_K;
// the padding is written as 0, which counts nothing.  A wave's store covers 256 consecutive bytes of one row.
//
// Gram (grm_gram_kernel<ATOMIC>): one wave per GRM_BLOCK x GRM_BLOCK block of pairs on or above the diagonal and per run of records.  The
// block is 2 x 2 tiles of v_mfma_i32_16x16x64_i8, five i32 accumulator tiles each: H Ht, H Lt, L Ht, L Lt and C Ct (80 accumulator
// registers).  The 16x16x64 form is used: its tile holds 4 accumulators per lane against 16 for 32x32x32, so a 32 x 32 block of five
// products costs 80 registers either way, and the smaller tile wastes less on the diagonal and on ragged cohorts.  A and B fragments come
// from the same image by the same rule -- lane l loads the 16 bytes at [row l & 15][k + 16 (l >> 4)] -- so whatever k order the
// instruction uses inside a step is the same on both sides.  C/D: column = lane & 15, row = 4 (lane >> 4) + register.
// |h h| <= 2^14 and a run is at most GRM_MAX_RUN = 65,536 records, so an i32 sum stays below 2^30.  At the end of its run the wave folds
//   S += 65536 HH + 256 (HL + LH) + LL,  N += CC
// into the 64-bit state of the pairs a <= b < n_samples, pair (a, b) at a (2 n - a + 1) / 2 + b - a.  ATOMIC: several runs share a block
// (a small cohort is split along the records) and add with 64-bit atomics -- integer sums do not depend on the order.  Otherwise a block
// has one wave in the launch and adds in place.
#pragma once
#include "grm_plan.h" // GRM_K, GRM_BLOCK, GRM_MAX_RUN, grm_run_plan (plain C++: malva_hip.hip includes it first, outside every namespace)
#include "ibd_kernels.h"

namespace {
using namespace mg;

constexpr u32 GRM_TPB = 256;
constexpr i32 GRM_SHIFT = 10, GRM_MAX_Q = 32639;
constexpr int GRM_SCRATCH_MB = 384; // a piece's three byte images at most (3 bytes per padded sample and record), unless one MFMA step needs more

struct GrmWeightArgs {
    u64 n_vars, v0, count; // the step's records (the stride of `sites`); the records to weigh: v0 .. v0 + count - 1, q_out[0 .. count - 1]
    u32 n_groups, n_samples;
    const unsigned long long *sites; // [n_groups][3][n_vars]
    int haploid;
    u32 maf_ppm, min_n;
};

// grid: ceil(count / GRM_TPB)
__global__ void __launch_bounds__(GRM_TPB) grm_weights_kernel(GrmWeightArgs a, short4 *__restrict__ q_out, unsigned long long *__restrict__ entered)
{
    const u64 t = (u64)blockIdx.x * GRM_TPB + threadIdx.x, v = a.v0 + t;
    bool enters = false;
    short4 q = make_short4(0, 0, 0, 0);
    if (t < a.count) {
        u32 n0 = 0, n1 = 0, n2 = 0;
        for (u32 g = 0; g < a.n_groups; ++g) {
            const u32 left = a.n_samples - 64 * g; // (n_groups == ceil(n_samples / 64): at least 1)
            const unsigned long long mask = left >= 64 ? ~0ull : (1ull << left) - 1ull;
            const unsigned long long *w = a.sites + (u64)g * 3 * a.n_vars + v;
            n0 += (u32)__popcll(w[0] & mask);
            n1 += (u32)__popcll(w[a.n_vars] & mask);
            n2 += (u32)__popcll(w[2 * a.n_vars] & mask);
        }
        long long n, an, ac, d;
        if (a.haploid) {
            n = n0 + n2, an = n, ac = n2;
            d = 4 * ac * (an - ac);
        } else {
            n = n0 + n1 + n2, an = 2 * n, ac = n1 + 2 * n2;
            d = 2 * ac * (an - ac);
        }
        if (d > 0) {
            const double root = __dsqrt_rn((double)d);
            long long qd[3];
            bool fits = true;
            for (int k = 0; k < 3; ++k) {
                qd[k] = (long long)rint(__ddiv_rn((double)((k * an - 2 * ac) * (1ll << GRM_SHIFT)), root));
                fits = fits && qd[k] <= GRM_MAX_Q && qd[k] >= -GRM_MAX_Q;
            }
            const long long minor = ac < an - ac ? ac : an - ac;
            enters = fits && n >= (long long)a.min_n && (unsigned long long)minor * 1000000ull >= (unsigned long long)a.maf_ppm * (unsigned long long)an;
            if (enters) q = make_short4((short)qd[0], (short)qd[1], (short)qd[2], 1);
        }
        q_out[t] = q;
    }
    if (entered) {
        const unsigned long long votes = __ballot(enters);
        if ((threadIdx.x & 63) == 0 && votes) atomicAdd(entered, (unsigned long long)__popcll(votes));
    }
}

struct GrmExpandArgs {
    u64 n_vars, v0, piece, ld; // the step's records; the piece's first record, its records, and its padded row (a multiple of GRM_K)
    u32 n_groups, n_samples, rows; // rows: the samples padded to GRM_BLOCK
    const unsigned long long *sites; // [n_groups][3][n_vars]
    const short4 *q;                 // [piece]
    int haploid;
    signed char *h, *l, *c;          // [rows][ld] each
};

// grid: (ceil(ld / 4 / GRM_TPB), ceil(rows / 64))
__global__ void __launch_bounds__(GRM_TPB) grm_expand_kernel(GrmExpandArgs a)
{
    const u64 r0 = ((u64)blockIdx.x * GRM_TPB + threadIdx.x) * 4; // (ld is a multiple of 4)
    if (r0 >= a.ld) return;
    const u32 g = blockIdx.y;
    unsigned long long w[4][3];
    i32 q[4][3];
#pragma unroll
    for (u32 r = 0; r < 4; ++r) {
        w[r][0] = w[r][1] = w[r][2] = 0;
        q[r][0] = q[r][1] = q[r][2] = 0;
        if (r0 + r < a.piece && g < a.n_groups) {
            const u64 v = a.v0 + r0 + r;
            const short4 qq = a.q[r0 + r];
            if (qq.w) {
                const u32 left = a.n_samples - 64 * g;
                const unsigned long long mask = left >= 64 ? ~0ull : (1ull << left) - 1ull;
                const unsigned long long *s = a.sites + (u64)g * 3 * a.n_vars + v;
                w[r][0] = s[0] & mask;
                w[r][1] = a.haploid ? 0ull : s[a.n_vars] & mask;
                w[r][2] = s[2 * a.n_vars] & mask;
                q[r][0] = qq.x, q[r][1] = qq.y, q[r][2] = qq.z;
            }
        }
    }
    for (u32 p = 0; p < 64; ++p) {
        const u32 row = 64 * g + p;
        if (row >= a.rows) break;
        u32 hw = 0, lw = 0, cw = 0;
#pragma unroll
        for (u32 r = 0; r < 4; ++r) {
            const u32 b0 = (u32)(w[r][0] >> p) & 1u, b1 = (u32)(w[r][1] >> p) & 1u, b2 = (u32)(w[r][2] >> p) & 1u;
            const i32 x = b0 ? q[r][0] : b1 ? q[r][1] : b2 ? q[r][2] : 0;
            const i32 lo = ((x + 128) & 255) - 128, hi = (x - lo) >> 8;
            hw |= ((u32)hi & 255u) << (8 * r);
            lw |= ((u32)lo & 255u) << (8 * r);
            cw |= (b0 | b1 | b2) << (8 * r);
        }
        const u64 at = (u64)row * a.ld + r0;
        *(u32 *)(a.h + at) = hw;
        *(u32 *)(a.l + at) = lw;
        *(u32 *)(a.c + at) = cw;
    }
}

struct GrmGramArgs {
    u64 ld, run;        // the padded row; records per wave, a multiple of GRM_K and at most GRM_MAX_RUN
    u32 n_samples;
    const signed char *h, *l, *c;
    long long *sum;            // [n (n + 1) / 2]
    unsigned long long *count; // likewise
};

typedef int grm_v4i __attribute__((ext_vector_type(4)));

// grid: (blocks, blocks, runs), blocks = rows / GRM_BLOCK; x runs along b; one wave
template <bool ATOMIC> __global__ void __launch_bounds__(64) grm_gram_kernel(GrmGramArgs a)
{
    const u32 bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return; // (workgroup-uniform)
    const u32 lane = threadIdx.x, r = lane & 15, kq = lane >> 4;
    const u64 k_begin = (u64)blockIdx.z * a.run, k_end = k_begin + a.run < a.ld ? k_begin + a.run : a.ld;
    const u64 row_a = ((u64)bi * GRM_BLOCK + r) * a.ld + 16 * kq, row_b = ((u64)bj * GRM_BLOCK + r) * a.ld + 16 * kq, next = 16 * a.ld;
    grm_v4i hh[2][2], hl[2][2], lh[2][2], ll[2][2], cc[2][2];
#pragma unroll
    for (u32 i = 0; i < 2; ++i)
#pragma unroll
        for (u32 j = 0; j < 2; ++j) hh[i][j] = hl[i][j] = lh[i][j] = ll[i][j] = cc[i][j] = grm_v4i{0, 0, 0, 0};
    for (u64 k = k_begin; k < k_end; k += GRM_K) {
        grm_v4i ah[2], al[2], ac[2], bh[2], bl[2], bc[2];
#pragma unroll
        for (u32 t = 0; t < 2; ++t) {
            ah[t] = *(const grm_v4i *)(a.h + row_a + t * next + k);
            al[t] = *(const grm_v4i *)(a.l + row_a + t * next + k);
            ac[t] = *(const grm_v4i *)(a.c + row_a + t * next + k);
            bh[t] = *(const grm_v4i *)(a.h + row_b + t * next + k);
            bl[t] = *(const grm_v4i *)(a.l + row_b + t * next + k);
            bc[t] = *(const grm_v4i *)(a.c + row_b + t * next + k);
        }
#pragma unroll
        for (u32 i = 0; i < 2; ++i)
#pragma unroll
            for (u32 j = 0; j < 2; ++j) {
                hh[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[i], bh[j], hh[i][j], 0, 0, 0);
                hl[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[i], bl[j], hl[i][j], 0, 0, 0);
                lh[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[i], bh[j], lh[i][j], 0, 0, 0);
                ll[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[i], bl[j], ll[i][j], 0, 0, 0);
                cc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac[i], bc[j], cc[i][j], 0, 0, 0);
            }
    }
    const u64 n = a.n_samples;
#pragma unroll
    for (u32 i = 0; i < 2; ++i)
#pragma unroll
        for (u32 j = 0; j < 2; ++j)
#pragma unroll
            for (u32 e = 0; e < 4; ++e) {
                const u64 sa = (u64)bi * GRM_BLOCK + 16 * i + 4 * kq + e, sb = (u64)bj * GRM_BLOCK + 16 * j + r;
                if (sa > sb || sb >= n) continue;
                const long long s = 65536ll * hh[i][j][e] + 256ll * ((long long)hl[i][j][e] + lh[i][j][e]) + ll[i][j][e];
                const unsigned long long cnt = (unsigned long long)(u32)cc[i][j][e];
                const u64 at = sa * (2 * n - sa + 1) / 2 + (sb - sa);
                if (ATOMIC) {
                    if (s) atomicAdd((unsigned long long *)a.sum + at, (unsigned long long)s);
                    if (cnt) atomicAdd(a.count + at, cnt);
                } else {
                    if (s) a.sum[at] += s;
                    if (cnt) a.count[at] += cnt;
                }
            }
}

} // namespace
