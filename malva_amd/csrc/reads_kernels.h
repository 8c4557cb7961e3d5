// reads_kernels.h -- the `kmc -k<ref_k> -ci -cs` step of the reference's pipeline (MALVA:104-110) on the device, fused
// into the call-time scan (main.cpp:482-500).  Included from malva_hip.hip inside its anonymous namespace, after
// scan_kernels.h.
//
// Reads arrive as ASCII chunks of whole records (one byte outside ACGT between records).  The chunk is packed as the
// reference is (pack_word: 2 bits per base + one bit per base outside ACGT, lower case folded), and every window of ref_k
// bases is made canonical and put to the scan's own gate test (row_gate_open).  A ref_k-mer whose window fails it cannot
// change a counter (BF::increment / KMAP::increment are no-ops then, bloom_filter.hpp:100-113, kmap.hpp:114-122), so it is
// dropped before it is counted.  The survivors are filed by a hash of the key into RD_PARTS partitions, counted one
// workgroup per partition (sort + run-length add in LDS), filtered by [min, max] and handed to the scan as an SoA table.
//
//   reads_window_kernel<MODE 0>  per chunk, as it arrives: windows -> survivors per partition (sizes the passes)
//   reads_window_kernel<MODE 1>  per pass: the survivors of the pass's partitions filed into their bins
//   reads_reduce_kernel          per pass, one workgroup per bin: the bin's distinct keys with their counts

constexpr int RD_PART_LOG2 = 18;
constexpr u32 RD_PARTS = 1u << RD_PART_LOG2; // key partitions = bins (a pass takes a contiguous range of them)
constexpr int RD_W = REF_SCAN_W;              // windows per thread (ref_scan_packed_kernel's loads)
constexpr int RD_TPB = 1024;                  // reduce: threads per workgroup
constexpr int RD_TILE = 4096;                 // reduce: pairs per LDS tile (84 KiB with the head flags)
constexpr int RD_PER = RD_TILE / RD_TPB;      // pairs per thread of a tile

__global__ void __launch_bounds__(TPB) reads_pack_kernel(const u8 *__restrict__ ascii, u64 n, u64 *__restrict__ codes, u32 *__restrict__ bad, u64 n_words)
{
    const u64 w = (u64)blockIdx.x * TPB + threadIdx.x;
    if (w >= n_words) return;
    pack_word<true>(ascii, n, w, codes, bad);
}

__device__ __forceinline__ u64 rd_mix(u64 x) // splitmix64's finaliser
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
// partition hash of a canonical ref_k-mer (M-form): the low RD_PART_LOG2 bits pick its bin, the high half its device
__device__ __forceinline__ u64 rd_key_hash(U128 m) { return rd_mix(m.lo ^ rd_mix(m.hi + 0x9E3779B97F4A7C15ULL)); }

struct ReadsPass {
    u32 part, n_parts;                // keep the keys with (hash >> 32) % n_parts == part
    u32 bin_mask;                     // partitions - 1 (RD_PARTS - 1; tests take fewer, to put many keys into one bin)
    u32 p_lo, p_hi;                   // MODE 1: partitions of this pass
    u32 *part_count;                  // MODE 0: [bin_mask + 1] survivors per partition
    const u64 *bin_base;              // MODE 1: [p_hi - p_lo] first pair of each bin
    u32 *bin_fill;                    // MODE 1: [p_hi - p_lo] pairs filed so far
    u64 *key_hi, *key_lo;             // MODE 1: the pairs' keys (their counts are 1)
    unsigned long long *meta;         // MODE 0: [0] windows without a base outside ACGT, [1] survivors
};

// One thread takes RD_W consecutive windows of a packed chunk (ref_scan_packed_kernel's loads: four code words and the bad
// bits of the span, the windows slid out of registers).  A window with a base outside ACGT -- N, the separator between two
// records, anything past the chunk's end -- is skipped, as KMC skips it.
template <int KC, int RC, int MODE>
__global__ void __launch_bounds__(TPB) reads_window_kernel(const u64 *__restrict__ codes, const u32 *__restrict__ badw, u64 n_windows, int k_rt, int r_rt,
                                                           BFView bf, ReadsPass rp)
{
    __shared__ u32 sh_lut[256];
    __shared__ unsigned long long sh_valid, sh_pass;
    ascii_lut_fill(sh_lut);
    if (threadIdx.x == 0) sh_valid = sh_pass = 0;
    __syncthreads();
    const int k = KC > 0 ? KC : k_rt, r = RC > 0 ? RC : r_rt;
    const int off = (r - k) / 2;
    const U128 mr = mask128(2 * r);
    const u64 bm_lo = r >= 64 ? ~0ULL : ((1ULL << r) - 1);
    u32 n_valid = 0, n_pass = 0;
    const u64 n_threads = (u64)gridDim.x * TPB;
    for (u64 t = (u64)blockIdx.x * TPB + threadIdx.x; t * RD_W < n_windows; t += n_threads) {
        const u64 w0 = t * RD_W;
        const u64 wi = w0 >> 5;
        const int o = (int)(w0 & 31) * 2;
        u64 q0 = codes[wi], q1 = codes[wi + 1], q2 = codes[wi + 2], q3 = codes[wi + 3];
        if (o) {
            q0 = (q0 >> o) | (q1 << (64 - o));
            q1 = (q1 >> o) | (q2 << (64 - o));
            q2 = (q2 >> o) | (q3 << (64 - o));
        }
        const u64 b01 = (u64)badw[wi] | ((u64)badw[wi + 1] << 32), b23 = (u64)badw[wi + 2] | ((u64)badw[wi + 3] << 32);
        const int ob = (int)(w0 & 31);
        const u64 blo = ob ? (b01 >> ob) | (b23 << (64 - ob)) : b01, bhi = b23 >> ob;
        for (int j = 0; j < RD_W; ++j) {
            if (w0 + j >= n_windows) break;
            if (shr128(U128{blo, bhi}, j).lo & bm_lo) continue;
            U128 L = shr128(U128{q0, q1}, 2 * j);
            if (j) L.hi |= q2 << (64 - 2 * j);
            L.lo &= mr.lo;
            L.hi &= mr.hi;
            ++n_valid;
            // canonical ref_k-mer (KMC -fm: the smaller of the window and its reverse complement), as an L-form and as the
            // M-form a table row holds: M(window) = the pair-reversed L-form; M(rc) = ~L(window), L(rc) = ~M(window)
            const U128 Lm = shr128(U128{pairrev64(L.hi), pairrev64(L.lo)}, 2 * (64 - r));
            const U128 Lrc{~Lm.lo & mr.lo, ~Lm.hi & mr.hi};
            const bool fw = !lt128(Lrc, L);
            const U128 cl = fw ? L : Lrc;
            const U128 cm = fw ? Lm : U128{~L.lo & mr.lo, ~L.hi & mr.hi};
            if (!row_gate_open<KC>(cm, cl, r, off, k, sh_lut, bf)) continue;
            const u64 h = rd_key_hash(cm);
            if (rp.n_parts > 1 && (u32)((h >> 32) % rp.n_parts) != rp.part) continue;
            const u32 p = (u32)h & rp.bin_mask;
            ++n_pass;
            if (MODE == 0) atomicAdd(&rp.part_count[p], 1u);
            else if (p >= rp.p_lo && p < rp.p_hi) {
                const u64 at = rp.bin_base[p - rp.p_lo] + atomicAdd(&rp.bin_fill[p - rp.p_lo], 1u);
                rp.key_hi[at] = cm.hi;
                rp.key_lo[at] = cm.lo;
            }
        }
    }
    if (MODE == 0) {
        if (n_valid) atomicAdd(&sh_valid, (unsigned long long)n_valid);
        if (n_pass) atomicAdd(&sh_pass, (unsigned long long)n_pass);
        __syncthreads();
        if (threadIdx.x == 0) {
            if (sh_valid) atomicAdd(&rp.meta[0], sh_valid);
            if (sh_pass) atomicAdd(&rp.meta[1], sh_pass);
        }
    }
}

struct ReadsReduce {
    const u64 *bin_base; // [bins] first pair of each bin
    const u32 *bin_n;    // [bins] pairs filed
    u64 *hi, *lo;        // the pairs: keys as filed, then rewritten in place by the tile rounds
    u32 *cnt;            // their counts once a tile round has run (before: 1 each)
    u32 min_count, max_count;
    u64 *out_hi, *out_lo; // the kept table (capacity: the pass's pairs)
    u32 *out_cnt;
    unsigned long long *out_n;
};

__device__ __forceinline__ bool rd_gt(u64 ah, u64 al, u64 bh, u64 bl) { return ah > bh || (ah == bh && al > bl); }

// exclusive prefix sum of one u32 per thread over the RD_TPB threads; *total = the sum (every thread of the workgroup calls it)
__device__ __forceinline__ u32 rd_block_scan(u32 v, u32 *sh_wave, u32 *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) sh_wave[wave] = x;
    __syncthreads();
    u32 before = 0, all = 0;
    for (int w = 0; w < RD_TPB / 64; ++w) {
        const u32 s = sh_wave[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads(); // (sh_wave is reused by the next call)
    *total = all;
    return before + x - v;
}

// one kept (key, count) per lane that takes it: one returning atomic per wave (every lane of the wave calls this)
__device__ __forceinline__ void rd_emit(bool take, u64 hi, u64 lo, u32 count, const ReadsReduce &rr)
{
    const u64 mask = __ballot(take);
    if (!mask) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((unsigned long long)mask) - 1;
    u32 base_lo = 0, base_hi = 0;
    if (lane == leader) {
        const unsigned long long b = atomicAdd(rr.out_n, (unsigned long long)__popcll(mask));
        base_lo = (u32)b;
        base_hi = (u32)(b >> 32);
    }
    const u64 base = (u64)__shfl(base_lo, leader, 64) | ((u64)__shfl(base_hi, leader, 64) << 32);
    if (take) {
        const u64 q = base + __popcll(mask & ((1ULL << lane) - 1));
        rr.out_hi[q] = hi;
        rr.out_lo[q] = lo;
        rr.out_cnt[q] = count;
    }
}

// Sort the m <= RD_TILE pairs in LDS (bitonic, padded to a power of two with the key ~0:~0, which no canonical ref_k-mer is --
// all-T's reverse complement is smaller), add up the counts of equal keys and leave the u distinct pairs at the front.
__device__ u32 rd_tile_reduce(u64 *sh_hi, u64 *sh_lo, u32 *sh_cnt, u8 *sh_head, u32 *sh_wave, u32 m)
{
    u32 size = 2;
    while (size < m) size <<= 1;
    for (u32 i = m + threadIdx.x; i < size; i += RD_TPB) {
        sh_hi[i] = sh_lo[i] = ~0ULL;
        sh_cnt[i] = 0;
    }
    __syncthreads();
    for (u32 s = 2; s <= size; s <<= 1)
        for (u32 st = s >> 1; st > 0; st >>= 1) {
            for (u32 p = threadIdx.x; p < size / 2; p += RD_TPB) {
                const u32 i = 2 * st * (p / st) + p % st, l = i + st;
                const bool asc = (i & s) == 0;
                if (rd_gt(sh_hi[i], sh_lo[i], sh_hi[l], sh_lo[l]) == asc) {
                    const u64 th = sh_hi[i], tl = sh_lo[i];
                    const u32 tc = sh_cnt[i];
                    sh_hi[i] = sh_hi[l];
                    sh_lo[i] = sh_lo[l];
                    sh_cnt[i] = sh_cnt[l];
                    sh_hi[l] = th;
                    sh_lo[l] = tl;
                    sh_cnt[l] = tc;
                }
            }
            __syncthreads();
        }
    for (u32 i = threadIdx.x; i < m; i += RD_TPB) sh_head[i] = i == 0 || sh_hi[i] != sh_hi[i - 1] || sh_lo[i] != sh_lo[i - 1];
    __syncthreads();
    u64 kh[RD_PER], kl[RD_PER];
    u32 kc[RD_PER], nh = 0;
#pragma unroll
    for (int q = 0; q < RD_PER; ++q) {
        const u32 i = threadIdx.x * RD_PER + q;
        if (i < m && sh_head[i]) {
            u64 sum = sh_cnt[i];
            for (u32 j = i + 1; j < m && !sh_head[j]; ++j) sum += sh_cnt[j];
            kh[nh] = sh_hi[i];
            kl[nh] = sh_lo[i];
            kc[nh] = (u32)(sum < 0xFFFFFFFFULL ? sum : 0xFFFFFFFFULL);
            ++nh;
        }
    }
    u32 total;
    const u32 at = rd_block_scan(nh, sh_wave, &total); // (its barriers also end every read of the tile above)
#pragma unroll
    for (int q = 0; q < RD_PER; ++q)
        if ((u32)q < nh) {
            sh_hi[at + q] = kh[q];
            sh_lo[at + q] = kl[q];
            sh_cnt[at + q] = kc[q];
        }
    __syncthreads();
    return total;
}

// One workgroup per bin.  Rounds of tiles: each tile of the bin sorted and run-length added in LDS and written back compacted
// (in place: a tile is read whole before anything is written, and nothing is written past what has been read), while a round
// shrinks the bin by a quarter or more -- repeats, high coverage and a satellite k-mer of any multiplicity collapse here.  A
// bin that fits one tile then finishes in LDS.  What stays larger (many distinct keys) is sorted in global memory by the same
// workgroup (bitonic network, +inf padding virtual) and its runs added.  Every loop is bounded by the bin's size: no lane ever
// waits on another.
__global__ void __launch_bounds__(RD_TPB) reads_reduce_kernel(ReadsReduce rr)
{
    __shared__ u64 sh_hi[RD_TILE], sh_lo[RD_TILE];
    __shared__ u32 sh_cnt[RD_TILE];
    __shared__ u8 sh_head[RD_TILE];
    __shared__ u32 sh_wave[RD_TPB / 64];
    const u64 base = rr.bin_base[blockIdx.x];
    u32 n = rr.bin_n[blockIdx.x];
    if (n == 0) return;
    u64 *H = rr.hi + base, *Lo = rr.lo + base;
    u32 *C = rr.cnt + base;
    bool ones = true; // the pairs are as filed: count 1 each, C not written yet
    auto load = [&](u32 t0, u32 m) {
        for (u32 i = threadIdx.x; i < m; i += RD_TPB) {
            sh_hi[i] = H[t0 + i];
            sh_lo[i] = Lo[t0 + i];
            sh_cnt[i] = ones ? 1u : C[t0 + i];
        }
        __syncthreads();
    };
    while (n > (u32)RD_TILE) {
        u32 w = 0;
        for (u32 t0 = 0; t0 < n; t0 += RD_TILE) {
            const u32 m = n - t0 < (u32)RD_TILE ? n - t0 : (u32)RD_TILE;
            load(t0, m);
            const u32 u = rd_tile_reduce(sh_hi, sh_lo, sh_cnt, sh_head, sh_wave, m);
            for (u32 i = threadIdx.x; i < u; i += RD_TPB) {
                H[w + i] = sh_hi[i];
                Lo[w + i] = sh_lo[i];
                C[w + i] = sh_cnt[i];
            }
            w += u;
            __syncthreads();
        }
        ones = false;
        const bool shrunk = w <= n - n / 4;
        n = w;
        if (!shrunk) break;
    }
    if (n <= (u32)RD_TILE) {
        load(0, n);
        const u32 u = rd_tile_reduce(sh_hi, sh_lo, sh_cnt, sh_head, sh_wave, n);
        for (u32 i0 = 0; i0 < u; i0 += RD_TPB) {
            const u32 i = i0 + threadIdx.x;
            const u32 c = i < u ? sh_cnt[i] : 0;
            rd_emit(i < u && c >= rr.min_count, i < u ? sh_hi[i] : 0, i < u ? sh_lo[i] : 0, c < rr.max_count ? c : rr.max_count, rr);
        }
        return;
    }
    // many distinct keys: bitonic sort of [0, n) in global memory (the flip form: every comparator ascending, so the padding up to
    // a power of two stays virtual -- a comparator that reaches past n is skipped), then one pass over the runs
    u32 size = 2;
    while (size < n) size <<= 1;
    auto cmpswap = [&](u32 i, u32 l) {
        const u64 ih = H[i], il = Lo[i], lh = H[l], ll = Lo[l];
        if (rd_gt(ih, il, lh, ll)) {
            const u32 ic = C[i];
            H[i] = lh;
            Lo[i] = ll;
            C[i] = C[l];
            H[l] = ih;
            Lo[l] = il;
            C[l] = ic;
        }
    };
    for (u32 s = 2; s <= size; s <<= 1) {
        const u32 half = s >> 1;
        for (u32 p = threadIdx.x; p < size / 2; p += RD_TPB) {
            const u32 b = p / half, j = p % half, i = b * s + j, l = b * s + s - 1 - j;
            if (l < n) cmpswap(i, l);
        }
        __syncthreads();
        for (u32 st = half >> 1; st > 0; st >>= 1) {
            for (u32 p = threadIdx.x; p < size / 2; p += RD_TPB) {
                const u32 i = 2 * st * (p / st) + p % st, l = i + st;
                if (l < n) cmpswap(i, l);
            }
            __syncthreads();
        }
    }
    for (u32 i0 = 0; i0 < n; i0 += RD_TPB) {
        const u32 i = i0 + threadIdx.x;
        const bool head = i < n && (i == 0 || H[i] != H[i - 1] || Lo[i] != Lo[i - 1]);
        u64 sum = 0;
        if (head) {
            sum = C[i];
            for (u32 j = i + 1; j < n && H[j] == H[i] && Lo[j] == Lo[i]; ++j) sum += C[j];
        }
        const u32 c = (u32)(sum < 0xFFFFFFFFULL ? sum : 0xFFFFFFFFULL);
        rd_emit(head && c >= rr.min_count, head ? H[i] : 0, head ? Lo[i] : 0, c < rr.max_count ? c : rr.max_count, rr);
    }
}
