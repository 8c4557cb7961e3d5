// The pair table of a multi-sample call set: for every pair of planes (samples) and every record where both are called, the joint
// count of their dosages, a 3 x 3 table per pair.  The reference -- one individual per run -- has nothing like it.
//
// Packing (mg_pack_dosage_device): pack_dosage_kernel turns the cells of a batch into bit planes, planes_out[plane][dosage][word],
// bit v & 63 of word v >> 6 set when the cell (plane, v) is a called cell of a biallelic record whose allele indexes are 0 or 1 and
// whose dosage is that one.  A wave takes 64 consecutive records of one plane: the arrays are plane-major, so its loads are
// coalesced; three ballots are the three words, and lanes 0..2 store one each.  Every word is written exactly once, by one wave:
// no atomics, no read-modify-write, and the bits of the last word at and behind n_vars come out 0 because those lanes vote false.
//
// Counting (mg_pair_counts_device): counts[i][j][3 da + db] = sum over w of popcount(A[i][da][w] & B[j][db][w]).  pair_count_kernel:
// a workgroup of PAIR_TILE x PAIR_TILE threads owns that many pairs and a run of words; thread (ti, tj) keeps its pair's nine sums
// in registers.  The run is staged PAIR_CHUNK words at a time into LDS as sa[d][w][i] and sb[d][w][j] -- the plane index innermost,
// rows padded to PAIR_LD -- so that in one ds_read_b64 of a 32-lane half the lanes that differ in j read 16 neighbouring 8-byte
// words (32 banks, each once) and the lanes that share i read one address (a broadcast); the two values of i in a half lie side by
// side.  The staging writes, consecutive lanes on consecutive words of one row, are PAIR_LD * 8 = 136 bytes apart: 2-way, twelve
// writes against 192 reads per thread and chunk.  The sums go to `counts` once, at the end, by 64-bit atomic adds: many workgroups
// along the word axis share an entry, and integer sums do not depend on the order.  B == A (planes_b NULL): the tiles below the
// diagonal are not computed; a tile above it adds its sums to the mirrored entries as well, transposed.
//
// 32-bit partial sums: a thread adds at most 64 per word to a sum, and a workgroup's run is at most PAIR_MAX_RUN = 2^20 words
// (pair_count_plan), so a sum stays below 2^26.
#pragma once
#include "call_text_kernels.h"
#include "count_plan.h" // PAIR_CHUNK, PAIR_MAX_RUN, pair_count_plan (plain C++: malva_hip.hip includes it first, outside every namespace)

namespace {
using namespace mg;

constexpr u32 PACK_TPB = 256;           // four waves, four words of one plane
constexpr u32 PAIR_TILE = 16;           // a workgroup's pairs: PAIR_TILE x PAIR_TILE, one per thread
constexpr u32 PAIR_TPB = PAIR_TILE * PAIR_TILE;
constexpr u32 PAIR_LD = PAIR_TILE + 1;  // the padded row of the LDS image
// LDS: 2 operands x 3 dosages x PAIR_CHUNK x PAIR_LD x 8 bytes = 26,112 bytes, static

struct PackArgs {
    u64 n_vars, n_words;
    u32 n_planes;
    int haploid;
    const i32 *gt1, *gt2, *gq; // [n_planes][n_vars]
    int use_mask;
    i32 min_gq;
    const u32 *var_allele_off; // [n_vars + 1]
};

// grid: (ceil(n_words / 4), n_planes)
__global__ void __launch_bounds__(PACK_TPB) pack_dosage_kernel(PackArgs a, unsigned long long *__restrict__ out)
{
    const u32 lane = threadIdx.x & 63;
    const u64 w = (u64)blockIdx.x * (PACK_TPB / 64) + (threadIdx.x >> 6);
    const u32 p = blockIdx.y;
    if (w >= a.n_words) return; // (wave-uniform)
    const u64 v = w * 64 + lane;
    u32 d = 3; // (no class)
    if (v < a.n_vars) {
        const u64 i = (u64)p * a.n_vars + v;
        const bool biallelic = a.var_allele_off[v + 1] - a.var_allele_off[v] == 2u;
        const u32 g1 = (u32)a.gt1[i], g2 = a.haploid ? g1 : (u32)a.gt2[i];
        bool called = true;
        if (a.use_mask) called = a.gq[i] >= a.min_gq;
        if (biallelic && called && g1 <= 1u && g2 <= 1u) d = g1 + g2; // (haploid: 2 * gt1)
    }
    const unsigned long long b0 = __ballot(d == 0u), b1 = __ballot(d == 1u), b2 = __ballot(d == 2u);
    if (lane < 3) out[((u64)p * 3 + lane) * a.n_words + w] = lane == 0 ? b0 : lane == 1 ? b1 : b2;
}

struct PairArgs {
    u64 n_words, run;                  // words per plane and dosage; words per workgroup (a multiple of PAIR_CHUNK)
    const unsigned long long *pa, *pb; // [n_a][3][n_words], [n_b][3][n_words]
    u32 n_a, n_b;
    int symmetric;                     // pb == pa: the tiles below the diagonal are left to their mirrors
};

// one operand's tile of a chunk: rows (plane, dosage) of PAIR_CHUNK words, read along the words, written plane-innermost.  A plane
// beyond the operand's last, a word at or beyond w_end: 0, which counts nothing.
__device__ __forceinline__ void pair_stage(unsigned long long (*s)[PAIR_CHUNK][PAIR_LD], const unsigned long long *planes, u32 n, u32 p0, u64 w0, u64 w_end, u64 n_words)
{
    const u32 cw = threadIdx.x % PAIR_CHUNK;
    for (u32 row = threadIdx.x / PAIR_CHUNK; row < 3 * PAIR_TILE; row += PAIR_TPB / PAIR_CHUNK) {
        const u32 pl = row / 3, d = row % 3;
        unsigned long long x = 0;
        if (p0 + pl < n && w0 + cw < w_end) x = planes[((u64)(p0 + pl) * 3 + d) * n_words + w0 + cw];
        s[d][cw][pl] = x;
    }
}

// grid: (word runs, tiles along j, tiles along i)
__global__ void __launch_bounds__(PAIR_TPB) pair_count_kernel(PairArgs a, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long sa[3][PAIR_CHUNK][PAIR_LD], sb[3][PAIR_CHUNK][PAIR_LD];
    const u32 tile_i = blockIdx.z, tile_j = blockIdx.y;
    if (a.symmetric && tile_j < tile_i) return; // (workgroup-uniform)
    const u32 ti = threadIdx.x / PAIR_TILE, tj = threadIdx.x % PAIR_TILE;
    const u64 w_begin = (u64)blockIdx.x * a.run, w_end = w_begin + a.run < a.n_words ? w_begin + a.run : a.n_words;
    u32 c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // (below 2^26: the head of this file)
    for (u64 w0 = w_begin; w0 < w_end; w0 += PAIR_CHUNK) {
        pair_stage(sa, a.pa, a.n_a, tile_i * PAIR_TILE, w0, w_end, a.n_words);
        pair_stage(sb, a.pb, a.n_b, tile_j * PAIR_TILE, w0, w_end, a.n_words);
        __syncthreads();
#pragma unroll 4
        for (u32 w = 0; w < PAIR_CHUNK; ++w) {
            const unsigned long long a0 = sa[0][w][ti], a1 = sa[1][w][ti], a2 = sa[2][w][ti];
            const unsigned long long b0 = sb[0][w][tj], b1 = sb[1][w][tj], b2 = sb[2][w][tj];
            c[0] += (u32)__popcll(a0 & b0); c[1] += (u32)__popcll(a0 & b1); c[2] += (u32)__popcll(a0 & b2);
            c[3] += (u32)__popcll(a1 & b0); c[4] += (u32)__popcll(a1 & b1); c[5] += (u32)__popcll(a1 & b2);
            c[6] += (u32)__popcll(a2 & b0); c[7] += (u32)__popcll(a2 & b1); c[8] += (u32)__popcll(a2 & b2);
        }
        __syncthreads();
    }
    const u32 i = tile_i * PAIR_TILE + ti, j = tile_j * PAIR_TILE + tj;
    if (i >= a.n_a || j >= a.n_b) return;
    unsigned long long *at = counts + ((u64)i * a.n_b + j) * 9;
    for (u32 k = 0; k < 9; ++k)
        if (c[k]) atomicAdd(at + k, (unsigned long long)c[k]);
    if (a.symmetric && tile_j != tile_i) { // the pair (j, i): the table transposed
        unsigned long long *mirror = counts + ((u64)j * a.n_b + i) * 9;
        for (u32 k = 0; k < 9; ++k)
            if (c[k]) atomicAdd(mirror + 3 * (k % 3) + k / 3, (unsigned long long)c[k]);
    }
}

} // namespace
