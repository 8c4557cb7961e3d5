// The LD table of a multi-sample call set: r2 between a record and the `window` records behind it, along the samples.  The reference -- one
// individual per run -- has nothing like it.
//
// Packing (mg_pack_site_dosage_device): pack_site_kernel makes sites_out[dosage][record], bit p set when the cell (p, record) contributes
// with that dosage -- the cell rule of pack_dosage_kernel (pair_kernels.h), the transposed layout.  A workgroup takes LD_PACK_RECS = 64
// consecutive records; a wave's lanes are those records in ONE plane, so every load is 256 consecutive bytes of a plane-major array, and
// the planes p = wave, wave + 4, ... are the wave's.  A lane ORs bit p into three words of its own; the four waves' words meet in LDS
// (4 x 3 x 64 words, 6 KB; written and read lane-consecutive, no conflict) and the first three waves store one dosage each, 512
// consecutive bytes.  Every word is written exactly once: no atomics.  64 planes in the 64 lanes would be site_geno_kernel's pattern, 64
// cache lines per load.
//
// Window (mg_ld_window_device): ld_window_kernel<WRITE>.  A workgroup owns LD_TILE = 16 records i, its four waves LD_R = 4 of them each;
// the offsets 1 .. window are walked in slabs of 64, lane = offset inside the slab.  So a thread keeps LD_R pairs (i0 + 4 wave + r,
// offset), all with the partner index jr = 4 wave + r + lane inside the slab's partner run of LD_TILE + 63 records, and per pair six
// 32-bit sums over the groups: n, |a1 B|, |a2 B|, |A b1|, |A b2| and Sxy (A = a0 | a1 | a2, the cells that contribute at i; B likewise at
// j) -- nine popcounts of 64-bit ANDs per pair and group.  With at most 2^14 samples every sum is below 2^17.
// A chunk of LD_GC groups is staged at a time: si[g][d][16] the tile's words, sj[g][d][LD_JN] the partner run's.  In one ds_read_b64 the
// lanes of a half-wave read 32 neighbouring 8-byte words of sj (64 banks, each once); the reads of si are one address per wave, a
// broadcast.  The staging reads are record-consecutive in global memory and in LDS.  A record at or beyond n_vars is staged as 0 and
// contributes nowhere.  LDS: LD_GC x 3 x (16 + 80) x 8 = 36,864 bytes, static.
// The ordered, compacted output: the length pass (WRITE = false) counts a record's emitted pairs -- a ballot per slab and record, the
// popcounts added up in a wave-uniform register -- into len[i]; the library's scan (fmt_scan) makes row_off; the write pass computes the
// same pairs again and puts a pair at row_off[i] + (the pairs of the slabs before) + (the ballot's bits below the lane).  No atomics, and
// the position depends on (i, offset) alone.  The dense alternative (keep the length pass' r2 for the write pass) costs
// n_first x window x 16 bytes of scratch and was not built.
//
// r2: cov = n Sxy - Sx Sy, vx = n Sxx - Sx Sx, vy = n Syy - Sy Sy in signed 64-bit (each at most 2^30 in magnitude, the products at most
// 2^60); r2 = double(u64(cov cov)) / double(u64(vx vy)): two conversions and one division, each correctly rounded (-ffp-contract=off).
#pragma once
#include "pair_kernels.h"

namespace {
using namespace mg;

constexpr u32 LD_PACK_TPB = 256, LD_PACK_RECS = 64;
constexpr u32 LD_TPB = 256, LD_R = 4, LD_TILE = (LD_TPB / 64) * LD_R; // 16 records i per workgroup
constexpr u32 LD_JN = 80;                                             // the partner run of a slab: LD_TILE + 63 records, rounded up
constexpr u32 LD_GC = 16;                                             // groups staged at a time
static_assert(LD_JN >= LD_TILE + 63, "the partner run");

// grid: ceil(n_vars / 64)
__global__ void __launch_bounds__(LD_PACK_TPB) pack_site_kernel(PackArgs a, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long sh[LD_PACK_TPB / 64][3][LD_PACK_RECS];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 v = (u64)blockIdx.x * LD_PACK_RECS + lane;
    unsigned long long w0 = 0, w1 = 0, w2 = 0;
    if (v < a.n_vars && a.var_allele_off[v + 1] - a.var_allele_off[v] == 2u) {
        for (u32 p = wave; p < a.n_planes; p += LD_PACK_TPB / 64) {
            const u64 i = (u64)p * a.n_vars + v;
            const u32 g1 = (u32)a.gt1[i], g2 = a.haploid ? g1 : (u32)a.gt2[i];
            bool called = true;
            if (a.use_mask) called = a.gq[i] >= a.min_gq;
            if (called && g1 <= 1u && g2 <= 1u) {
                const u32 d = g1 + g2; // (haploid: 2 * gt1)
                const unsigned long long bit = 1ull << p;
                w0 |= d == 0u ? bit : 0ull;
                w1 |= d == 1u ? bit : 0ull;
                w2 |= d == 2u ? bit : 0ull;
            }
        }
    }
    sh[wave][0][lane] = w0;
    sh[wave][1][lane] = w1;
    sh[wave][2][lane] = w2;
    __syncthreads();
    if (wave < 3 && v < a.n_vars) out[(u64)wave * a.n_vars + v] = sh[0][wave][lane] | sh[1][wave][lane] | sh[2][wave][lane] | sh[3][wave][lane];
}

struct LdArgs {
    u64 n_vars, n_first;
    u32 n_groups, window;
    const unsigned long long *sites; // [n_groups][3][n_vars]
    const u32 *chrom, *pos;          // [n_vars]
    u64 max_bp;
    u32 min_n;
    double min_r2;
};

struct LdPair { // mg_ld_pair
    u32 i, j, n;
    i32 sign;
    double r2;
};
static_assert(sizeof(LdPair) == 24, "mg_ld_pair is 24 bytes");

// grid: ceil(n_first / LD_TILE).  WRITE = false: len[i] = record i's emitted pairs.  WRITE = true: the pairs, at row_off[i] onwards,
// none at or behind cap.
template <bool WRITE>
__global__ void __launch_bounds__(LD_TPB) ld_window_kernel(LdArgs a, u32 *__restrict__ len, const unsigned long long *__restrict__ row_off, LdPair *__restrict__ out,
                                                          u64 cap)
{
    __shared__ unsigned long long si[LD_GC][3][LD_TILE], sj[LD_GC][3][LD_JN];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 i0 = (u64)blockIdx.x * LD_TILE;
    u32 emitted[LD_R] = {0, 0, 0, 0}; // (wave-uniform) the pairs of the slabs so far
    for (u32 s0 = 0; s0 < a.window; s0 += 64) {
        const u64 j0 = i0 + 1 + s0; // the slab's first partner; partner jr is record j0 + jr
        if (j0 >= a.n_vars) break;  // (workgroup-uniform) no partner left in this or a later slab
        u32 sn[LD_R], sa1[LD_R], sa2[LD_R], sb1[LD_R], sb2[LD_R], sxy[LD_R];
#pragma unroll
        for (u32 r = 0; r < LD_R; ++r) sn[r] = sa1[r] = sa2[r] = sb1[r] = sb2[r] = sxy[r] = 0;
        for (u32 g0 = 0; g0 < a.n_groups; g0 += LD_GC) {
            const u32 gc = a.n_groups - g0 < LD_GC ? a.n_groups - g0 : LD_GC;
            for (u32 t = threadIdx.x; t < gc * 3 * LD_TILE; t += LD_TPB) {
                const u32 row = t / LD_TILE, ir = t % LD_TILE;
                const u64 v = i0 + ir;
                si[row / 3][row % 3][ir] = v < a.n_vars ? a.sites[((u64)(g0 + row / 3) * 3 + row % 3) * a.n_vars + v] : 0ull;
            }
            for (u32 t = threadIdx.x; t < gc * 3 * LD_JN; t += LD_TPB) {
                const u32 row = t / LD_JN, jr = t % LD_JN;
                const u64 v = j0 + jr;
                sj[row / 3][row % 3][jr] = v < a.n_vars ? a.sites[((u64)(g0 + row / 3) * 3 + row % 3) * a.n_vars + v] : 0ull;
            }
            __syncthreads();
            for (u32 g = 0; g < gc; ++g) {
#pragma unroll
                for (u32 r = 0; r < LD_R; ++r) {
                    const u32 ir = wave * LD_R + r, jr = ir + lane;
                    const unsigned long long a0 = si[g][0][ir], a1 = si[g][1][ir], a2 = si[g][2][ir];
                    const unsigned long long b0 = sj[g][0][jr], b1 = sj[g][1][jr], b2 = sj[g][2][jr];
                    const unsigned long long A = a0 | a1 | a2, B = b0 | b1 | b2;
                    sn[r] += (u32)__popcll(A & B);
                    sa1[r] += (u32)__popcll(a1 & B);
                    sa2[r] += (u32)__popcll(a2 & B);
                    sb1[r] += (u32)__popcll(A & b1);
                    sb2[r] += (u32)__popcll(A & b2);
                    sxy[r] += (u32)__popcll(a1 & b1) + 2u * ((u32)__popcll(a1 & b2) + (u32)__popcll(a2 & b1)) + 4u * (u32)__popcll(a2 & b2);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (u32 r = 0; r < LD_R; ++r) {
            const u64 i = i0 + wave * LD_R + r, j = i + 1 + s0 + lane;
            bool emit = i < a.n_first && s0 + lane < a.window && j < a.n_vars && sn[r] >= a.min_n;
            if (emit) emit = a.chrom[i] == a.chrom[j];
            if (emit && a.max_bp) {
                const long long d = (long long)a.pos[j] - (long long)a.pos[i];
                emit = (u64)(d < 0 ? -d : d) <= a.max_bp;
            }
            const long long n = sn[r], sx = (long long)sa1[r] + 2 * (long long)sa2[r], sxx = (long long)sa1[r] + 4 * (long long)sa2[r];
            const long long sy = (long long)sb1[r] + 2 * (long long)sb2[r], syy = (long long)sb1[r] + 4 * (long long)sb2[r];
            const long long cov = n * (long long)sxy[r] - sx * sy, vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
            double r2 = 0.0;
            emit = emit && vx > 0 && vy > 0;
            if (emit) {
                r2 = (double)(unsigned long long)(cov * cov) / (double)(unsigned long long)(vx * vy);
                emit = r2 >= a.min_r2;
            }
            const unsigned long long votes = __ballot(emit);
            if (WRITE) {
                if (emit) {
                    const u64 at = row_off[i] + emitted[r] + (u32)__popcll(votes & ((1ull << lane) - 1ull));
                    if (at < cap) out[at] = LdPair{(u32)i, (u32)j, sn[r], cov > 0 ? 1 : cov < 0 ? -1 : 0, r2};
                }
            }
            emitted[r] += (u32)__popcll(votes);
        }
    }
    if (!WRITE && lane == 0) {
#pragma unroll
        for (u32 r = 0; r < LD_R; ++r) {
            const u64 i = i0 + wave * LD_R + r;
            if (i < a.n_first) len[i] = emitted[r];
        }
    }
}

} // namespace
