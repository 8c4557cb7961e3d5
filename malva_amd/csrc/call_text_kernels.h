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
    const u32 *var_allele_off;   // [n_vars + 1] (with cov)
    int masked;                  // mg_format_calls_masked: a cell whose gq < min_gq prints its genotype as missing ('.' or './.')
    i32 min_gq;
};

// plane p's cell of record v, the tab in front of it included
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
    return len;
}
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
    return pos;
}

// meta[1] is raised when a row does not fit 32 bits (the scan then reports ~0 as the total)
__global__ void __launch_bounds__(FMT_TPB) fmt_len_kernel(FmtArgs a, u32 *__restrict__ len, unsigned long long *meta)
{
    const u32 lane = threadIdx.x & 63;
    const u64 v = (u64)blockIdx.x * (FMT_TPB / 64) + (threadIdx.x >> 6);
    if (v >= a.n_vars) return;
    unsigned long long mine = lane < a.n_planes ? fmt_cell_len(a, v, lane) : 0;
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
struct FmtCellRows {
    FmtArgs a;
    __device__ __forceinline__ void put(const FmtWindow &w, u64 v, u32 lane, u64 r0, u64 r1) const
    {
        const u32 mine = lane < a.n_planes ? fmt_cell_len(a, v, lane) : 0;
        u32 incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 up = (u32)__shfl_up((int)incl, d, 64);
            if (lane >= (u32)d) incl += up;
        }
        const u64 at = r0 + (incl - mine);
        if (lane < a.n_planes && at < w.w0 + w.wlen && at + mine > w.w0) fmt_cell_put(a, w, v, lane, at);
        if (lane == 0) w.put(r1 - 1, '\n');
    }
};

__global__ void __launch_bounds__(FMT_TPB) fmt_write_kernel(FmtArgs a, const unsigned long long *__restrict__ row_off, char *text, u64 text_cap)
{
    __shared__ __attribute__((aligned(16))) char sh[FMT_WINDOW];
    fmt_write_tile(FmtCellRows{a}, sh, a.n_vars, row_off, text, text_cap);
}

} // namespace
