// IBS0-free segments per pair of samples: where along the records two samples share genotypes.  The reference -- one individual per
// run -- has nothing like it.  The definition is in include/malva_hip.h (mg_ibd_step); tests/ibd_model.py restates it.
//
// Transpose (mg_sites_to_planes_device): sites_to_planes_kernel turns the groups' site words, sites[group][dosage][record] with bits over
// samples (pack_site_kernel, ld_kernels.h), into the bit planes of pack_dosage_kernel (pair_kernels.h), planes[64 group + p][dosage][word]
// with bits over records -- in the order of `sites`, which a caller keeps in merged-file order.  A workgroup takes IBD_TR_WORDS = 16
// neighbouring word indexes of one (group, dosage); a wave takes four of them: its lanes load 64 consecutive records' words (512
// consecutive bytes) of each, __ballot((word >> p) & 1) is plane p's word, and lane p keeps it.  The 64 x 16 words meet in
// LDS (rows padded to 17: the lanes' writes are 136 bytes apart, 2-way, as pair_stage's) and leave as 64 runs of 128 bytes, one per
// plane.  Every word of every plane is written exactly once: no atomics; a record at or beyond n_vars is loaded as 0.
//
// Chromosome starts (ibd_starts_kernel): bit v & 63 of starts[v >> 6] is set when chrom[v] differs from chrom[v - 1], record 0 being
// compared with the last record of the step before (*last).  A wave per word, one ballot.
//
// Walk (ibd_walk_kernel<WRITE>): one thread per pair (a, b), a < b, in PAIR_TILE x PAIR_TILE tiles; the tiles below the diagonal leave at
// once.  The chunk's words are staged through LDS by pair_stage, PAIR_CHUNK at a time, with the start words beside them.  A pair's state
// -- chrom, start_pos, end_pos, n, ibs2; n == 0 means closed, an open run has at least one record -- lives in registers for the call and in
// five u32 arrays [n_pairs] between calls, pair (a, b) at a (2 n - a - 1) / 2 + b - a - 1: the threads of a tile row are neighbours there.
// Per word:  A = a0 | a1 | a2, B likewise, C = A & B;  D = (a0 & b2) | (a2 & b0) the opposite homozygotes;  I2 = (a0 & b0) | (a1 & b1) |
// (a2 & b2);  CONC = C & ~D  (I2 is a subset of it).  A run is broken in front of every bit of K = D | S, S the start word.  K == 0, the
// fast path: the word is one piece -- two popcounts, a ctz where the run opens, a clz for its last record.  Otherwise the pieces between
// K's bits are walked one by one, the run closed between them; a record of S that is CONC opens the next piece, one of D belongs to none.
// pos[] is read where a run opens, where it closes, and behind the chunk's last word for a run still open (its last record's index is
// kept meanwhile); chrom[] where a run opens.
// The ordered output, without atomics: the length pass (WRITE = false) counts a pair's closed segments into len[pair] and stores no
// state; the library's scan (fmt_scan) makes the offsets; the write pass walks again, puts the pair's segments at off[pair] onwards in
// the order it closes them, and stores the state.  The host runs the write pass only when the buffer holds the total.
#pragma once
#include "ld_kernels.h"

namespace {
using namespace mg;

constexpr u32 IBD_TR_TPB = 256, IBD_TR_WORDS = 16, IBD_TR_LD = IBD_TR_WORDS + 1;
constexpr u32 IBD_FIELDS = 5; // the state's arrays: chrom, start_pos, end_pos, n, ibs2

// grid: (ceil(n_words / IBD_TR_WORDS), 3, n_groups)
__global__ void __launch_bounds__(IBD_TR_TPB) sites_to_planes_kernel(const unsigned long long *__restrict__ sites, u64 n_vars, u64 n_words,
                                                                    unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long sh[64][IBD_TR_LD];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 g = blockIdx.z, d = blockIdx.y;
    const u64 w_first = (u64)blockIdx.x * IBD_TR_WORDS;
    const unsigned long long *src = sites + ((u64)g * 3 + d) * n_vars;
    constexpr u32 Q = IBD_TR_WORDS / (IBD_TR_TPB / 64); // a wave's word indexes, taken together: one `lane == p` serves all of them
    unsigned long long x[Q], mine[Q];
#pragma unroll
    for (u32 q = 0; q < Q; ++q) {
        const u64 v = (w_first + wave * Q + q) * 64 + lane;
        x[q] = v < n_vars ? src[v] : 0ull;
        mine[q] = 0;
    }
#pragma unroll
    for (u32 p = 0; p < 64; ++p) {
        const bool me = lane == p;
#pragma unroll
        for (u32 q = 0; q < Q; ++q) {
            const unsigned long long word = __ballot((x[q] >> p) & 1ull);
            if (me) mine[q] = word;
        }
    }
#pragma unroll
    for (u32 q = 0; q < Q; ++q) sh[lane][wave * Q + q] = mine[q];
    __syncthreads();
    for (u32 t = threadIdx.x; t < 64 * IBD_TR_WORDS; t += IBD_TR_TPB) {
        const u32 p = t / IBD_TR_WORDS, wi = t % IBD_TR_WORDS;
        if (w_first + wi < n_words) out[((u64)(64 * g + p) * 3 + d) * n_words + w_first + wi] = sh[p][wi];
    }
}

// grid: ceil(n_words / 4)
__global__ void __launch_bounds__(256) ibd_starts_kernel(const u32 *__restrict__ chrom, u64 n_vars, u64 n_words, const u32 *__restrict__ last,
                                                         unsigned long long *__restrict__ starts)
{
    const u32 lane = threadIdx.x & 63;
    const u64 w = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_words) return; // (wave-uniform)
    const u64 v = w * 64 + lane;
    bool starts_here = false;
    if (v < n_vars) starts_here = chrom[v] != (v ? chrom[v - 1] : *last);
    const unsigned long long word = __ballot(starts_here);
    if (lane == 0) starts[w] = word;
}

struct IbdArgs {
    u64 n_vars, n_words, n_pairs;
    u32 n_samples;
    const unsigned long long *planes; // [64 n_groups][3][n_words]
    const unsigned long long *starts; // [n_words]
    const u32 *chrom, *pos;           // [n_vars]
    u32 *state;                       // [IBD_FIELDS][n_pairs]
    u32 min_records;
    long long min_bp;
    int flush;
};

struct IbdSeg { // mg_ibd_seg
    u32 a, b, chrom, start_pos, end_pos, n, ibs2, zero;
};
static_assert(sizeof(IbdSeg) == 32, "mg_ibd_seg is 32 bytes");

// grid: (tiles, tiles), tiles = ceil(n_samples / PAIR_TILE); x runs along b.  WRITE = false: len[pair] = the segments the pair closes.
// WRITE = true: the segments, at off[pair] onwards, and the pair's new state.
template <bool WRITE>
__global__ void __launch_bounds__(PAIR_TPB) ibd_walk_kernel(IbdArgs a, u32 *__restrict__ len, const unsigned long long *__restrict__ off, IbdSeg *__restrict__ out)
{
    __shared__ unsigned long long sa[3][PAIR_CHUNK][PAIR_LD], sb[3][PAIR_CHUNK][PAIR_LD], ss[PAIR_CHUNK];
    const u32 tile_i = blockIdx.y, tile_j = blockIdx.x;
    if (tile_j < tile_i) return; // (workgroup-uniform)
    const u32 ti = threadIdx.x / PAIR_TILE, tj = threadIdx.x % PAIR_TILE;
    const u32 pa = tile_i * PAIR_TILE + ti, pb = tile_j * PAIR_TILE + tj;
    const bool valid = pa < pb && pb < a.n_samples;
    const u64 k = valid ? (u64)pa * (2ull * a.n_samples - pa - 1) / 2 + (pb - pa - 1) : 0;
    u32 chrom = 0, start = 0, end = 0, n = 0, ibs2 = 0;
    if (valid) {
        chrom = a.state[k];
        start = a.state[a.n_pairs + k];
        end = a.state[2 * a.n_pairs + k];
        n = a.state[3 * a.n_pairs + k];
        ibs2 = a.state[4 * a.n_pairs + k];
    }
    long long end_rec = -1; // the open run's last record in this call; -1: `end` holds its position
    u32 closed = 0;
    const u64 at = WRITE && valid ? off[k] : 0;
    auto close = [&]() {
        if (n) {
            const u32 e = end_rec >= 0 ? a.pos[end_rec] : end;
            if (n >= a.min_records && (long long)e - (long long)start >= a.min_bp) {
                if (WRITE) out[at + closed] = IbdSeg{pa, pb, chrom, start, e, n, ibs2, 0u};
                ++closed;
            }
            n = 0;
            end_rec = -1;
        }
    };
    auto piece = [&](u64 base, unsigned long long pc, unsigned long long same) {
        if (!n) {
            const u64 first = base + (u32)__builtin_ctzll(pc);
            chrom = a.chrom[first];
            start = a.pos[first];
            ibs2 = 0;
        }
        n += (u32)__popcll(pc);
        ibs2 += (u32)__popcll(same);
        end_rec = (long long)(base + 63u - (u32)__builtin_clzll(pc));
    };
    for (u64 w0 = 0; w0 < a.n_words; w0 += PAIR_CHUNK) {
        pair_stage(sa, a.planes, a.n_samples, tile_i * PAIR_TILE, w0, a.n_words, a.n_words);
        pair_stage(sb, a.planes, a.n_samples, tile_j * PAIR_TILE, w0, a.n_words, a.n_words);
        if (threadIdx.x < PAIR_CHUNK) ss[threadIdx.x] = w0 + threadIdx.x < a.n_words ? a.starts[w0 + threadIdx.x] : 0ull;
        __syncthreads();
        if (valid) {
            for (u32 w = 0; w < PAIR_CHUNK; ++w) {
                const unsigned long long a0 = sa[0][w][ti], a1 = sa[1][w][ti], a2 = sa[2][w][ti];
                const unsigned long long b0 = sb[0][w][tj], b1 = sb[1][w][tj], b2 = sb[2][w][tj];
                const unsigned long long C = (a0 | a1 | a2) & (b0 | b1 | b2), D = (a0 & b2) | (a2 & b0), I2 = (a0 & b0) | (a1 & b1) | (a2 & b2);
                const unsigned long long conc = C & ~D;
                unsigned long long K = D | ss[w];
                const u64 base = (w0 + w) * 64;
                if (!K) {
                    if (conc) piece(base, conc, I2);
                    continue;
                }
                u32 lo = 0; // (below 64: a break bit's own index)
                for (;;) {
                    const u32 hi = K ? (u32)__builtin_ctzll(K) : 64u;
                    const unsigned long long mask = (hi == 64u ? ~0ull : (1ull << hi) - 1ull) & (~0ull << lo); // records [lo, hi)
                    if (conc & mask) piece(base, conc & mask, I2 & mask);
                    if (hi == 64u) break;
                    close();
                    K &= K - 1ull;
                    lo = hi;
                }
            }
        }
        __syncthreads();
    }
    if (!valid) return;
    if (a.flush) close();
    if (!WRITE) {
        len[k] = closed;
        return;
    }
    if (n && end_rec >= 0) end = a.pos[end_rec];
    a.state[k] = chrom;
    a.state[a.n_pairs + k] = start;
    a.state[2 * a.n_pairs + k] = end;
    a.state[3 * a.n_pairs + k] = n;
    a.state[4 * a.n_pairs + k] = ibs2;
}

} // namespace
