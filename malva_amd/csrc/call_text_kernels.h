// The sample columns of a multi-sample VCF made on the device: the GT/GQ print of VB::output_variants (var_block.hpp:337-396),
// which the reference -- one individual per run -- does once per record, repeated here for every plane of a cohort.
//
// A merged record is its fixed columns once and then one `GT:GQ` cell per sample.  The cells are all that differs between the
// samples, and their numbers ([planes][n_vars] gt1 / gt2 / gq, optionally the per-allele coverages) are what the genotype calls
// leave: so row v -- for every plane in order a tab and the cell, then '\n' -- is made here, and the host splices it behind the
// record's prefix instead of formatting planes x records lines with std::to_string.
//
// Three steps (mg_format_calls_device):
//   fmt_len_kernel     one wave per record, lane = plane: the lane's cell length, summed over the wave -> len[v]
//   the scan           len[] -> row_off[] (u64) and the total: tile_reduce_kernel + part_scan_kernel of store_kernels.h, then
//                      fmt_rescan_kernel (tile_rescan_kernel with 64-bit results)
//   fmt_write_kernel   a workgroup per FMT_ROWS consecutive records, whose rows are one contiguous byte range of the output: the
//                      range is staged in LDS a window at a time -- one wave per record, every lane its cell at the offset a wave
//                      prefix sum gives it -- with the window laid out at the output's own misalignment, so that it leaves in
//                      aligned 16-byte stores.  Only the pieces a tile shares with its neighbours (its first and last, and the one
//                      text_cap cuts) are stored byte by byte.
// Numbers print as std::to_string(int) prints them over the whole int32 range; a coverage as std::to_string((int)cov).
//
// MG_CELLS_GP adds the field GP behind the cell's last: the record's normalised likelihoods (`probs`, the doubles behind GTS= of the
// single-sample output) in VCF genotype order, each printed as printf("%f") prints it.  A value is 8 bytes (`0.dddddd`, `1.000000`) when it
// is printable -- sign bit clear and <= 1 -- and the one byte `.` when it is not, so the length pass formats nothing; the digits are made
// in integers from the double's bits (gp_micro), to nearest on the exact value with ties to even, as glibc rounds.
//
// MG_CELLS_PL adds the field PL behind the cell's last (behind GP, which is optional there): the G integers of `pl` (what
// mg_phred_likelihoods leaves: already in VCF order, copied and not permuted), each as std::to_string(int) prints it, `.` for
// MG_PL_MISSING; the whole field is one `.` when G == 0 or every value of the cell is missing.  Any other int32 is a value: the encoder
// does not know where the numbers came from.  A masked cell keeps its PL.
#pragma once
#include "kmer_dev.h"

namespace {
using namespace mg;

constexpr int FMT_TPB = 256;
constexpr int FMT_ROWS = 32;      // records per workgroup of the write pass (typical rows of 0.1 - 0.5 KB: one window)
constexpr int FMT_WINDOW = 16384; // bytes of the output staged at a time (a multiple of 16)

__device__ __forceinline__ u32 fmt_int_len(i32 v)
{
    const u32 m = v < 0 ? 0u - (u32)v : (u32)v;
    u32 nd = 1;
    nd += m >= 10u; nd += m >= 100u; nd += m >= 1000u; nd += m >= 10000u; nd += m >= 100000u;
    nd += m >= 1000000u; nd += m >= 10000000u; nd += m >= 100000000u; nd += m >= 1000000000u;
    return nd + (v < 0);
}

// the bytes of the output that lie in [w0, w0 + wlen) land in LDS at their offset from w0 (+ mis: see fmt_write_kernel)
struct FmtWindow {
    char *lds;
    u64 w0;
    u32 wlen;
    __device__ __forceinline__ void put(u64 pos, char b) const
    {
        const u64 rel = pos - w0;
        if (rel < (u64)wlen) lds[rel] = b;
    }
    // std::to_string(int); returns the position behind it
    __device__ __forceinline__ u64 put_int(u64 pos, i32 v) const
    {
        const u32 len = fmt_int_len(v);
        u32 m = v < 0 ? 0u - (u32)v : (u32)v;
        if (v < 0) put(pos, '-');
        u64 at = pos + len;
        do {
            put(--at, (char)('0' + m % 10u));
            m /= 10u;
        } while (m);
        return pos + len;
    }
};

struct FmtArgs {
    u64 n_vars;
    u32 n_planes;
    int haploid;
    const i32 *gt1, *gt2, *gq;   // [n_planes][n_vars]
    const u32 *cov;              // [n_planes][var_allele_off[n_vars]] or NULL
    const u32 *var_allele_off;   // [n_vars + 1] (with cov or probs)
    int masked;                  // mg_cells.use_mask: a cell whose gq < min_gq prints its genotype as missing ('.' or './.')
    i32 min_gq;
    // MG_CELLS_GP (all three or none; var_allele_off is then required with or without cov)
    const double *probs;         // [n_planes][var_gt_off[n_vars]], a record's values in the reference's order: a outer, c >= a inner
    const u64 *var_gt_off;       // [n_vars + 1]
    const u8 *status;            // [n_planes][n_vars]: a cell that is not MG_GT_NORMAL has no list, its probs are not read
    // MG_CELLS_PL (with var_allele_off and var_gt_off; probs and status then both or neither)
    const i32 *pl;               // [n_planes][var_gt_off[n_vars]], a record's values in VCF order
};

constexpr i32 FMT_PL_MISSING = INT32_MIN; // MG_PL_MISSING

// ---- GP: the genotype posteriors of a cell -----------------------------------------------------------------------------------------
// printable: sign bit clear and 0 <= p <= 1 (as bit patterns the non-negative doubles are ordered like integers: NaN, +inf and
// everything above 1 lie behind 1.0, whatever has its sign bit set -- -0.0 included -- behind those)
__device__ __forceinline__ bool gp_printable(double p) { return (u64)__double_as_longlong(p) <= 0x3FF0000000000000ull; }

// a printable p in millionths, rounded to nearest on the exact binary value, ties to even: what printf("%f") prints without its point.
// p = m 2^-s with m the 53-bit significand (a denormal's without the hidden bit), s = 1075 - the biased exponent (1074 for denormals):
// N = m 10^6 (< 2^73, two words), q = N >> s, r = N mod 2^s against half = 2^(s-1).  s >= 128: q = 0 and r = N < half.
__device__ __forceinline__ u32 gp_micro(double p)
{
    const u64 bits = (u64)__double_as_longlong(p);
    const u32 e = (u32)(bits >> 52);
    const u64 m = e ? (bits & 0xFFFFFFFFFFFFFull) | 1ull << 52 : bits;
    const u32 s = 1075u - (e ? e : 1u); // 52 .. 1074
    if (s >= 128) return 0;
    const u64 lo = m * 1000000ull, hi = __umul64hi(m, 1000000ull);
    u64 q, r_hi, r_lo, h_hi, h_lo;
    if (s < 64) {
        q = hi << (64 - s) | lo >> s;
        r_hi = 0;
        r_lo = lo & ((1ull << s) - 1);
        h_hi = 0;
        h_lo = 1ull << (s - 1);
    } else {
        const u32 t = s - 64;
        q = hi >> t;
        r_hi = hi & ((1ull << t) - 1);
        r_lo = lo;
        h_hi = t ? 1ull << (t - 1) : 0;
        h_lo = t ? 0 : 1ull << 63;
    }
    if (r_hi > h_hi || (r_hi == h_hi && r_lo > h_lo)) q += 1;
    else if (r_hi == h_hi && r_lo == h_lo) q += q & 1;
    return (u32)q;
}

// where genotype j/k (j <= k) of a diploid record of A alleles lies in probs' order
__device__ __forceinline__ u64 gp_src(u32 A, u32 j, u32 k) { return (u64)j * (2ull * A - j + 1) / 2 + (k - j); }

// the bytes of a cell's GP field, its ':' included
__device__ __forceinline__ u32 gp_len(const FmtArgs &a, u64 v, u32 p)
{
    if (a.status[(u64)p * a.n_vars + v] != MG_GT_NORMAL) return 2;
    const u64 A = a.var_allele_off[v + 1] - a.var_allele_off[v], G = a.haploid ? A : A * (A + 1) / 2;
    const double *pr = a.probs + (u64)p * a.var_gt_off[a.n_vars] + a.var_gt_off[v];
    u32 len = G ? 0 : 1;
    for (u64 g = 0; g < G; ++g) len += gp_printable(pr[g]) ? 9 : 2; // (':' in front of the first, ',' of the others; the order does not matter here)
    return len;
}
// A value whose bytes lie wholly outside the window is stepped over by its width alone; behind the window's end nothing is left to do.
__device__ __forceinline__ u64 gp_put(const FmtArgs &a, const FmtWindow &w, u64 v, u32 p, u64 pos)
{
    w.put(pos++, ':');
    if (a.status[(u64)p * a.n_vars + v] != MG_GT_NORMAL) {
        w.put(pos++, '.');
        return pos;
    }
    const u32 A = a.var_allele_off[v + 1] - a.var_allele_off[v];
    const double *pr = a.probs + (u64)p * a.var_gt_off[a.n_vars] + a.var_gt_off[v];
    const u64 w1 = w.w0 + w.wlen;
    bool first = true;
    for (u32 k = 0; k < A; ++k)
        for (u32 j = a.haploid ? k : 0; j <= k; ++j) { // VCF order: index k (k + 1) / 2 + j; haploid: the allele
            if (pos >= w1) return pos;
            if (!first) w.put(pos++, ',');
            first = false;
            const double x = pr[a.haploid ? (u64)k : gp_src(A, j, k)];
            if (!gp_printable(x)) {
                w.put(pos++, '.');
                continue;
            }
            if (pos + 8 <= w.w0 || pos >= w1) {
                pos += 8;
                continue;
            }
            u32 q = gp_micro(x);
            w.put(pos, q == 1000000u ? '1' : '0');
            w.put(pos + 1, '.');
            if (q == 1000000u) q = 0;
            for (u32 d = 8; d-- > 2;) {
                w.put(pos + d, (char)('0' + q % 10u));
                q /= 10u;
            }
            pos += 8;
        }
    return pos;
}

// ---- PL: the Phred-scaled likelihoods of a cell ------------------------------------------------------------------------------------------
// the bytes of a cell's PL field, its ':' included
__device__ __forceinline__ u32 pl_len(const FmtArgs &a, u64 v, u32 p)
{
    const u64 A = a.var_allele_off[v + 1] - a.var_allele_off[v], G = a.haploid ? A : A * (A + 1) / 2;
    const i32 *pl = a.pl + (u64)p * a.var_gt_off[a.n_vars] + a.var_gt_off[v];
    u32 len = 0;
    bool any = false;
    for (u64 g = 0; g < G; ++g) {
        const i32 x = pl[g];
        any |= x != FMT_PL_MISSING;
        len += 1 + (x == FMT_PL_MISSING ? 1u : fmt_int_len(x)); // (':' in front of the first, ',' of the others)
    }
    return any ? len : 2;
}
__device__ __forceinline__ u64 pl_put(const FmtArgs &a, const FmtWindow &w, u64 v, u32 p, u64 pos)
{
    const u64 A = a.var_allele_off[v + 1] - a.var_allele_off[v], G = a.haploid ? A : A * (A + 1) / 2;
    const i32 *pl = a.pl + (u64)p * a.var_gt_off[a.n_vars] + a.var_gt_off[v];
    const u64 w1 = w.w0 + w.wlen;
    bool any = false;
    for (u64 g = 0; g < G && !any; ++g) any = pl[g] != FMT_PL_MISSING;
    w.put(pos++, ':');
    if (!any) {
        w.put(pos++, '.');
        return pos;
    }
    for (u64 g = 0; g < G; ++g) {
        if (pos >= w1) return pos; // (behind the window's end nothing is left to do)
        if (g) w.put(pos++, ',');
        const i32 x = pl[g];
        if (x == FMT_PL_MISSING) w.put(pos++, '.');
        else pos = w.put_int(pos, x);
    }
    return pos;
}

// plane p's cell of record v, the tab in front of it included.  GP: the kernels under MG_CELLS_GP -- a build of their own, so that
// those of the entries without it keep the registers they had; PL: those under MG_CELLS_PL, for the same reason
template <bool GP, bool PL = false>
__device__ __forceinline__ u32 fmt_cell_len(const FmtArgs &a, u64 v, u32 p)
{
    const u64 i = (u64)p * a.n_vars + v;
    const i32 gq = a.gq[i];
    u32 len = 1 + 1 + fmt_int_len(gq);
    if (a.masked && gq < a.min_gq) len += a.haploid ? 1 : 3;
    else {
        len += fmt_int_len(a.gt1[i]);
        if (!a.haploid) len += 1 + fmt_int_len(a.gt2[i]);
    }
    if (a.cov) {
        const u32 a0 = a.var_allele_off[v], a1 = a.var_allele_off[v + 1];
        const u32 *cv = a.cov + (u64)p * a.var_allele_off[a.n_vars];
        for (u32 s = a0; s < a1; ++s) len += 1 + fmt_int_len((i32)cv[s]); // (':' in front of the first, ',' of the others)
        if (a0 == a1) len += 1;                                          // a record without alleles: the empty list behind its ':'
    }
    if (GP) len += gp_len(a, v, p);
    if (PL) len += pl_len(a, v, p);
    return len;
}
template <bool GP, bool PL = false>
__device__ __forceinline__ u64 fmt_cell_put(const FmtArgs &a, const FmtWindow &w, u64 v, u32 p, u64 pos)
{
    const u64 i = (u64)p * a.n_vars + v;
    const i32 gq = a.gq[i];
    w.put(pos++, '\t');
    if (a.masked && gq < a.min_gq) {
        w.put(pos++, '.');
        if (!a.haploid) {
            w.put(pos++, '/');
            w.put(pos++, '.');
        }
    } else {
        pos = w.put_int(pos, a.gt1[i]);
        if (!a.haploid) {
            w.put(pos++, '/');
            pos = w.put_int(pos, a.gt2[i]);
        }
    }
    w.put(pos++, ':');
    pos = w.put_int(pos, gq);
    if (a.cov) {
        const u32 a0 = a.var_allele_off[v], a1 = a.var_allele_off[v + 1];
        const u32 *cv = a.cov + (u64)p * a.var_allele_off[a.n_vars];
        if (a0 == a1) w.put(pos++, ':');
        for (u32 s = a0; s < a1; ++s) {
            w.put(pos++, s == a0 ? ':' : ',');
            pos = w.put_int(pos, (i32)cv[s]);
        }
    }
    if (GP) pos = gp_put(a, w, v, p, pos);
    if (PL) pos = pl_put(a, w, v, p, pos);
    return pos;
}

// meta[1] is raised when a row does not fit 32 bits (the scan then reports ~0 as the total)
template <bool GP, bool PL = false>
__global__ void __launch_bounds__(FMT_TPB) fmt_len_kernel(FmtArgs a, u32 *__restrict__ len, unsigned long long *meta)
{
    const u32 lane = threadIdx.x & 63;
    const u64 v = (u64)blockIdx.x * (FMT_TPB / 64) + (threadIdx.x >> 6);
    if (v >= a.n_vars) return;
    unsigned long long mine = lane < a.n_planes ? fmt_cell_len<GP, PL>(a, v, lane) : 0;
    for (int d = 32; d; d >>= 1) mine += (unsigned long long)__shfl_xor((long long)mine, d, 64);
    if (lane == 0) {
        mine += 1; // '\n'
        if (mine > 0xFFFFFFFFull) atomicOr(meta + 1, 1ull);
        len[v] = (u32)mine;
    }
}

// tile_rescan_kernel (store_kernels.h) with 64-bit results: off[i] = sum of x[0 .. i), off[n] = the total (~0 when meta[1] is set)
__global__ void __launch_bounds__(SCAN_TPB) fmt_rescan_kernel(const u32 *__restrict__ x, u64 n, const unsigned long long *__restrict__ part,
                                                              unsigned long long *__restrict__ off, unsigned long long *meta)
{
    __shared__ unsigned long long sh16[SCAN_TPB / 64];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK;
    unsigned long long carry = part[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = 0; j < SCAN_PER; ++j) {
        const u64 i = base + (u64)j * SCAN_TPB + threadIdx.x;
        const u32 v = i < n ? x[i] : 0u;
        unsigned long long incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = (unsigned long long)__shfl_up((long long)incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) sh16[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, round_total = 0;
        for (int w = 0; w < SCAN_TPB / 64; ++w) {
            if (w < wave) before += sh16[w];
            round_total += sh16[w];
        }
        if (i < n) off[i] = carry + before + incl - v;
        carry += round_total;
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        off[n] = carry;
        if (meta[1]) meta[0] = ~0ull;
    }
}

// the window's bytes [w0, stop) leave: LDS bytes [mis, mis + stop - w0), whole 16-byte pieces at once and the ragged ends byte by byte
__device__ __forceinline__ void fmt_window_flush(const char *sh, u32 mis, char *text, u64 w0, u64 stop)
{
    const u32 lo = mis, hi = mis + (u32)(stop - w0);
    char *dst = text + w0 - mis; // 16-byte aligned
    for (u32 j = threadIdx.x; j * 16 < hi; j += FMT_TPB) {
        const u32 p0 = j * 16;
        if (p0 >= lo && p0 + 16 <= hi) *reinterpret_cast<uint4 *>(dst + p0) = *reinterpret_cast<const uint4 *>(sh + p0);
        else
            for (u32 q = p0 < lo ? lo : p0; q < p0 + 16 && q < hi; ++q) dst[q] = sh[q];
    }
}

// The write pass of one workgroup: rows [t0, t1) are one contiguous byte range of the output, staged in `sh` (FMT_WINDOW bytes, 16-byte
// aligned) a window at a time.  rows.put(w, v, lane, r0, r1) has one wave lay row v = bytes [r0, r1) into the window (FmtWindow::put drops
// what lies outside it).
template <class Rows>
__device__ __forceinline__ void fmt_write_tile(const Rows &rows, char *sh, u64 n_rows, const unsigned long long *__restrict__ row_off, char *text, u64 text_cap)
{
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 t0 = (u64)blockIdx.x * FMT_ROWS;
    const u64 t1 = t0 + FMT_ROWS < n_rows ? t0 + FMT_ROWS : n_rows;
    const u64 b0 = row_off[t0], b1 = row_off[t1];
    const u64 end = b1 < text_cap ? b1 : text_cap; // nothing is written at or behind text_cap
    for (u64 w0 = b0; w0 < end;) {
        // the window starts at LDS byte `mis`, the output address's offset in its 16-byte piece, and ends with a piece unless the tile does
        const u32 mis = (u32)((uintptr_t)(text + w0) & 15);
        const u64 w1 = b1 - w0 < (u64)(FMT_WINDOW - mis) ? b1 : w0 + (FMT_WINDOW - mis);
        const FmtWindow w{sh + mis, w0, (u32)(w1 - w0)};
        for (u64 v = t0 + wave; v < t1; v += FMT_TPB / 64) {
            const u64 r0 = row_off[v], r1 = row_off[v + 1];
            if (r1 <= w0 || r0 >= w1) continue; // (wave-uniform)
            rows.put(w, v, lane, r0, r1);
        }
        __syncthreads();
        fmt_window_flush(sh, mis, text, w0, w1 < end ? w1 : end);
        __syncthreads(); // (the next window overwrites sh)
        w0 = w1;
    }
}

// a record's sample columns: every lane its plane's cell at the offset a wave prefix sum gives it
template <bool GP, bool PL = false>
struct FmtCellRows {
    FmtArgs a;
    __device__ __forceinline__ void put(const FmtWindow &w, u64 v, u32 lane, u64 r0, u64 r1) const
    {
        const u32 mine = lane < a.n_planes ? fmt_cell_len<GP, PL>(a, v, lane) : 0;
        u32 incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 up = (u32)__shfl_up((int)incl, d, 64);
            if (lane >= (u32)d) incl += up;
        }
        const u64 at = r0 + (incl - mine);
        if (lane < a.n_planes && at < w.w0 + w.wlen && at + mine > w.w0) fmt_cell_put<GP, PL>(a, w, v, lane, at);
        if (lane == 0) w.put(r1 - 1, '\n');
    }
};

template <bool GP, bool PL = false>
__global__ void __launch_bounds__(FMT_TPB) fmt_write_kernel(FmtArgs a, const unsigned long long *__restrict__ row_off, char *text, u64 text_cap)
{
    __shared__ __attribute__((aligned(16))) char sh[FMT_WINDOW];
    fmt_write_tile(FmtCellRows<GP, PL>{a}, sh, a.n_vars, row_off, text, text_cap);
}

} // namespace
