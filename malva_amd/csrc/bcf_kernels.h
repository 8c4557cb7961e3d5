// The sample columns of a multi-sample BCF made on the device: per record the bytes of BCF2's per-sample ("indiv") block (VCF/BCF
// specification v4.3, section 6.3.3) -- what call_text_kernels.h makes as text, here in the binary form, 3 bytes per diploid GT:GQ cell
// instead of 8 to 10.  Restated from the published layout; no file written by htslib exists here: parity unpinned, as for the reader.
//
// Row v = for each of its two fields (three with cov, one more with probs: MG_CELLS_GP), in this order:
//   GT    typed_int(key_gt)  desc(ploidy, T)  [plane][ploidy] values   ploidy 1 (haploid) or 2; allele index a -> (a + 1) << 1 (unphased)
//   GQ    typed_int(key_gq)  desc(1, T)       [plane] values           as they are, mask or no mask
//   COVS  typed_int(key_cov) desc(A, T)       [plane][A] values        (int32_t)cov[..], A = the record's alleles
//   GP    typed_int(key_gp)  desc(G, 5)       [plane][G] float32       the record's likelihoods in VCF genotype order, G = A (haploid) or
//                                                                      A (A + 1) / 2; (float)p to nearest even, made in integers (gp_float_bits)
//                                                                      so that float denormals stay; an unprintable value (gp_printable)
//                                                                      is the missing float, a cell that is not MG_GT_NORMAL the missing
//                                                                      float and G - 1 end-of-vector floats
//   PL    typed_int(key_pl)  desc(G, T)       [plane][G] values        MG_CELLS_PL (GP is optional there): `pl` as it comes, already in
//                                                                      VCF order; T the smallest type that holds every value of the field that
//                                                                      is not MG_PL_MISSING (int8 when there is none); MG_PL_MISSING is T's missing
//                                                                      code (0x80, 0x8000, 0x80000000), a cell whose values are all missing that
//                                                                      code and G - 1 end-of-vector codes (0x81, 0x8001, 0x80000001)
// desc(n, t) is the byte n << 4 | t for n < 15, else 0xF0 | t and typed_int(n); typed_int(x) is desc(1, t) and x in the smallest of int8
// (t = 1), int16 (2), int32 (3) that holds it; little endian throughout.  T of a field of a record is the smallest type that holds
// every value of that field over all planes with BCF's reserved codes (missing, end of vector) kept free: int8 for [-120, 127], int16
// for [-32760, 32767], else int32.  An int32 value inside int32's own reserved range [INT_MIN, INT_MIN + 7] is written as it is: what
// it then means to a reader is the caller's business.  A field without values (COVS of a record without alleles) is int8.
//
// Where the binary form departs from the text: a masked cell (gq < min_gq) writes 0 -- BCF's missing allele -- for each of its values,
// and so does an allele index outside [0, 2^30 - 2], whose code would not fit; mg_format_calls prints such an index as it is.
//
// Three steps (mg_encode_calls_bcf_device), those of mg_format_calls:
//   bcf_len_kernel     one wave per record, lane = plane: wave min / max of the GT codes, of GQ and (the lanes looping over the
//                      record's alleles) of the coverages -> the three type codes types[3 v ..] and the row length len[v]
//                      (GP is float32 whatever its values: its share of the length is arithmetic, probs are not read)
//   the scan           fmt_scan: len[] -> row_off[] (u64) and the total
//   bcf_write_kernel   fmt_write_tile with BcfRows: the field headers by lane 0, every lane its plane's values at an offset that is
//                      pure arithmetic (no prefix sum: the cells of a field are of one width), through the same LDS window and
//                      aligned 16-byte stores
#pragma once
#include "call_text_kernels.h"

namespace {
using namespace mg;

struct BcfArgs {
    u64 n_vars;
    u32 n_planes;
    int haploid;
    const i32 *gt1, *gt2, *gq;   // [n_planes][n_vars]
    const u32 *cov;              // [n_planes][var_allele_off[n_vars]] or NULL
    const u32 *var_allele_off;   // [n_vars + 1] (with cov or probs)
    int masked;
    i32 min_gq;
    i32 key_gt, key_gq, key_cov; // dictionary indexes, >= 0
    // MG_CELLS_GP (all three or none, as FmtArgs')
    const double *probs;         // [n_planes][var_gt_off[n_vars]]
    const u64 *var_gt_off;       // [n_vars + 1]
    const u8 *status;            // [n_planes][n_vars]
    i32 key_gp;
    // MG_CELLS_PL (with var_allele_off and var_gt_off; probs and status then both or neither)
    const i32 *pl;               // [n_planes][var_gt_off[n_vars]]
    i32 key_pl;
};

constexpr u32 BCF_FLOAT_MISSING = 0x7F800001u, BCF_FLOAT_EOV = 0x7F800002u;

// (float)p of a printable p as bits, round to nearest even, without the conversion instruction (whose treatment of a denormal result
// hangs on the kernel's mode): p = M 2^(e - 1075); a float's unit is 2^(e - 1046) where it is normal (e >= 897), else 2^-149
__device__ __forceinline__ u32 gp_float_bits(double p)
{
    const u64 bits = (u64)__double_as_longlong(p);
    const u32 e = (u32)(bits >> 52);
    if (e <= 862) return 0; // below 2^-160 (zero and the double denormals included): less than half the smallest float
    const u64 M = (bits & 0xFFFFFFFFFFFFFull) | 1ull << 52;
    const u32 sh = e >= 897 ? 29u : 926u - e; // 29 .. 63
    u32 f = (e >= 897 ? (e - 897) << 23 : 0u) + (u32)(M >> sh); // (a normal's hidden bit adds the exponent's last 1)
    const u64 r = M & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    if (r > half || (r == half && (f & 1))) ++f; // (a carry out of the mantissa is the next exponent)
    return f;
}

__device__ __forceinline__ u32 bcf_type_of(i32 lo, i32 hi)
{
    if (lo >= -120 && hi <= 127) return 1;
    if (lo >= -32760 && hi <= 32767) return 2;
    return 3;
}
__device__ __forceinline__ u32 bcf_width(u32 t) { return t == 3 ? 4u : t; }
__device__ __forceinline__ u32 bcf_typed_int_len(i32 x) { return 1 + bcf_width(bcf_type_of(x, x)); }
__device__ __forceinline__ u32 bcf_desc_len(u32 n) { return n < 15 ? 1 : 1 + bcf_typed_int_len((i32)n); }
// the value an allele index is written as
__device__ __forceinline__ i32 bcf_gt_code(i32 a, bool masked) { return masked || a < 0 || a > 0x3FFFFFFE ? 0 : (a + 1) << 1; }

__device__ __forceinline__ u64 bcf_put_val(const FmtWindow &w, u64 pos, i32 v, u32 t)
{
    w.put(pos, (char)v);
    if (t >= 2) w.put(pos + 1, (char)((u32)v >> 8));
    if (t == 3) {
        w.put(pos + 2, (char)((u32)v >> 16));
        w.put(pos + 3, (char)((u32)v >> 24));
    }
    return pos + bcf_width(t);
}
__device__ __forceinline__ u64 bcf_put_typed_int(const FmtWindow &w, u64 pos, i32 x)
{
    const u32 t = bcf_type_of(x, x);
    w.put(pos, (char)(0x10 | t));
    return bcf_put_val(w, pos + 1, x, t);
}
__device__ __forceinline__ u64 bcf_put_desc(const FmtWindow &w, u64 pos, u32 n, u32 t)
{
    if (n < 15) {
        w.put(pos, (char)(n << 4 | t));
        return pos + 1;
    }
    w.put(pos, (char)(0xF0 | t));
    return bcf_put_typed_int(w, pos + 1, (i32)n);
}

__device__ __forceinline__ i32 bcf_wave_min(i32 x)
{
    for (int d = 32; d; d >>= 1) {
        const i32 y = __shfl_xor(x, d, 64);
        x = y < x ? y : x;
    }
    return x;
}
__device__ __forceinline__ i32 bcf_wave_max(i32 x)
{
    for (int d = 32; d; d >>= 1) {
        const i32 y = __shfl_xor(x, d, 64);
        x = y > x ? y : x;
    }
    return x;
}

// the bytes of row v whose three fields have the types t[0..2] (t[2] unused without cov).  GP: the kernels under MG_CELLS_GP, a
// build of their own as in call_text_kernels.h
template <bool GP, bool PL = false>
__device__ __forceinline__ u64 bcf_row_len(const BcfArgs &a, u64 v, const u32 *t)
{
    const u64 P = a.n_planes;
    u64 len = bcf_typed_int_len(a.key_gt) + 1 + P * (a.haploid ? 1u : 2u) * bcf_width(t[0]);
    len += bcf_typed_int_len(a.key_gq) + 1 + P * bcf_width(t[1]);
    if (a.cov) {
        const u32 A = a.var_allele_off[v + 1] - a.var_allele_off[v];
        len += bcf_typed_int_len(a.key_cov) + bcf_desc_len(A) + P * A * bcf_width(t[2]);
    }
    if (GP) {
        const u64 A = a.var_allele_off[v + 1] - a.var_allele_off[v], G = a.haploid ? A : A * (A + 1) / 2;
        len += bcf_typed_int_len(a.key_gp) + bcf_desc_len((u32)G) + P * G * 4;
    }
    if (PL) {
        const u64 A = a.var_allele_off[v + 1] - a.var_allele_off[v], G = a.haploid ? A : A * (A + 1) / 2;
        len += bcf_typed_int_len(a.key_pl) + bcf_desc_len((u32)G) + P * G * bcf_width(t[3]);
    }
    return len;
}

// meta[1] is raised when a row does not fit 32 bits, as by fmt_len_kernel.  A record has three type codes, four with PL (BCF_TYPES)
template <bool PL>
constexpr u32 BCF_TYPES = PL ? 4 : 3;
template <bool GP, bool PL = false>
__global__ void __launch_bounds__(FMT_TPB) bcf_len_kernel(BcfArgs a, u32 *__restrict__ len, unsigned char *__restrict__ types, unsigned long long *meta)
{
    const u32 lane = threadIdx.x & 63;
    const u64 v = (u64)blockIdx.x * (FMT_TPB / 64) + (threadIdx.x >> 6);
    if (v >= a.n_vars) return; // (wave-uniform)
    // (a lane without a plane holds what no minimum and no maximum picks)
    i32 g_lo = INT32_MAX, g_hi = INT32_MIN, q_lo = INT32_MAX, q_hi = INT32_MIN, c_lo = INT32_MAX, c_hi = INT32_MIN;
    if (lane < a.n_planes) {
        const u64 i = (u64)lane * a.n_vars + v;
        const i32 gq = a.gq[i];
        const bool m = a.masked && gq < a.min_gq;
        const i32 c1 = bcf_gt_code(a.gt1[i], m), c2 = a.haploid ? c1 : bcf_gt_code(a.gt2[i], m);
        g_lo = c1 < c2 ? c1 : c2;
        g_hi = c1 < c2 ? c2 : c1;
        q_lo = q_hi = gq;
        if (a.cov) {
            const u32 a0 = a.var_allele_off[v], a1 = a.var_allele_off[v + 1];
            const u32 *cv = a.cov + (u64)lane * a.var_allele_off[a.n_vars];
            for (u32 s = a0; s < a1; ++s) {
                const i32 x = (i32)cv[s];
                c_lo = x < c_lo ? x : c_lo;
                c_hi = x > c_hi ? x : c_hi;
            }
        }
    }
    u32 t[BCF_TYPES<PL>];
    t[0] = bcf_type_of(bcf_wave_min(g_lo), bcf_wave_max(g_hi));
    t[1] = bcf_type_of(bcf_wave_min(q_lo), bcf_wave_max(q_hi));
    t[2] = 1;
    if (a.cov) {
        c_lo = bcf_wave_min(c_lo);
        c_hi = bcf_wave_max(c_hi);
        if (c_lo <= c_hi) t[2] = bcf_type_of(c_lo, c_hi); // (else: a record without alleles)
    }
    if (PL) {
        i32 p_lo = INT32_MAX, p_hi = INT32_MIN;
        if (lane < a.n_planes) {
            const u64 A = a.var_allele_off[v + 1] - a.var_allele_off[v], G = a.haploid ? A : A * (A + 1) / 2;
            const i32 *pl = a.pl + (u64)lane * a.var_gt_off[a.n_vars] + a.var_gt_off[v];
            for (u64 g = 0; g < G; ++g) {
                const i32 x = pl[g];
                if (x == FMT_PL_MISSING) continue;
                p_lo = x < p_lo ? x : p_lo;
                p_hi = x > p_hi ? x : p_hi;
            }
        }
        p_lo = bcf_wave_min(p_lo);
        p_hi = bcf_wave_max(p_hi);
        t[BCF_TYPES<PL> - 1] = p_lo <= p_hi ? bcf_type_of(p_lo, p_hi) : 1; // (else: no value that is not missing)
    }
    if (lane < BCF_TYPES<PL>) types[BCF_TYPES<PL> * v + lane] = (unsigned char)(lane == 0 ? t[0] : lane == 1 ? t[1] : lane == 2 ? t[2] : t[BCF_TYPES<PL> - 1]);
    if (lane == 0) {
        const u64 bytes = bcf_row_len<GP, PL>(a, v, t);
        if (bytes > 0xFFFFFFFFull) atomicOr(meta + 1, 1ull);
        len[v] = (u32)bytes;
    }
}

// a record's row: the field headers by lane 0, the values of plane `lane` by that lane
template <bool GP, bool PL = false>
struct BcfRows {
    BcfArgs a;
    const unsigned char *types;
    __device__ __forceinline__ void put(const FmtWindow &w, u64 v, u32 lane, u64 r0, u64) const
    {
        constexpr u32 NT = BCF_TYPES<PL>;
        const u32 t_gt = types[NT * v], t_gq = types[NT * v + 1], t_cov = types[NT * v + 2];
        const u32 ploidy = a.haploid ? 1 : 2;
        const bool mine = lane < a.n_planes;
        const u64 i = (u64)lane * a.n_vars + v;
        const i32 gq = mine ? a.gq[i] : 0;
        // GT
        u64 pos = r0;
        if (lane == 0) bcf_put_desc(w, bcf_put_typed_int(w, pos, a.key_gt), ploidy, t_gt);
        pos += bcf_typed_int_len(a.key_gt) + 1;
        if (mine) {
            const bool m = a.masked && gq < a.min_gq;
            u64 at = pos + (u64)lane * ploidy * bcf_width(t_gt);
            at = bcf_put_val(w, at, bcf_gt_code(a.gt1[i], m), t_gt);
            if (!a.haploid) bcf_put_val(w, at, bcf_gt_code(a.gt2[i], m), t_gt);
        }
        pos += (u64)a.n_planes * ploidy * bcf_width(t_gt);
        // GQ
        if (lane == 0) bcf_put_desc(w, bcf_put_typed_int(w, pos, a.key_gq), 1, t_gq);
        pos += bcf_typed_int_len(a.key_gq) + 1;
        if (mine) bcf_put_val(w, pos + (u64)lane * bcf_width(t_gq), gq, t_gq);
        pos += (u64)a.n_planes * bcf_width(t_gq);
        const u64 w1 = w.w0 + w.wlen;
        if (a.cov) { // COVS
            const u32 a0 = a.var_allele_off[v], A = a.var_allele_off[v + 1] - a0;
            if (lane == 0) bcf_put_desc(w, bcf_put_typed_int(w, pos, a.key_cov), A, t_cov);
            pos += bcf_typed_int_len(a.key_cov) + bcf_desc_len(A);
            const u64 span = (u64)A * bcf_width(t_cov);
            u64 at = pos + (u64)lane * span;
            if (mine && at < w1 && at + span > w.w0) { // (else: nothing of this plane's in the window)
                const u32 *cv = a.cov + (u64)lane * a.var_allele_off[a.n_vars] + a0;
                for (u32 s = 0; s < A; ++s) at = bcf_put_val(w, at, (i32)cv[s], t_cov);
            }
            pos += (u64)a.n_planes * span;
        }
        if (GP) pos = put_gp(w, v, lane, mine, i, pos);
        if (PL) put_pl(w, v, lane, mine, types[NT * v + NT - 1], pos);
    }
    // GP: value g of this plane at pos + (lane G + g) 4 -- only those of the window are loaded; returns the position behind the field
    __device__ __forceinline__ u64 put_gp(const FmtWindow &w, u64 v, u32 lane, bool mine, u64 i, u64 pos) const
    {
        const u64 w1 = w.w0 + w.wlen;
        const u32 A = a.var_allele_off[v + 1] - a.var_allele_off[v];
        const u64 G = a.haploid ? (u64)A : (u64)A * (A + 1) / 2;
        if (lane == 0) bcf_put_desc(w, bcf_put_typed_int(w, pos, a.key_gp), (u32)G, 5);
        pos += bcf_typed_int_len(a.key_gp) + bcf_desc_len((u32)G);
        const u64 at = pos + (u64)lane * G * 4, behind = pos + (u64)a.n_planes * G * 4;
        if (!mine || at >= w1 || at + G * 4 <= w.w0) return behind;
        const u64 g_lo = w.w0 > at ? (w.w0 - at) / 4 : 0, g_hi = w1 - at < G * 4 ? (w1 - at + 3) / 4 : G; // (a value the window cuts is made on both sides)
        const bool normal = a.status[i] == MG_GT_NORMAL;
        const double *pr = a.probs + (u64)lane * a.var_gt_off[a.n_vars] + a.var_gt_off[v];
        // VCF index g = k (k + 1) / 2 + j: (j, k) of g_lo from a square root, put right in integers, then stepped
        u32 k = 0, j = 0;
        if (!a.haploid && normal) {
            k = (u32)((sqrt(8.0 * (double)g_lo + 1.0) - 1.0) / 2.0);
            while ((u64)k * (k + 1) / 2 > g_lo) --k;
            while ((u64)(k + 1) * (k + 2) / 2 <= g_lo) ++k;
            j = (u32)(g_lo - (u64)k * (k + 1) / 2);
        }
        for (u64 g = g_lo; g < g_hi; ++g) {
            u32 f = g ? BCF_FLOAT_EOV : BCF_FLOAT_MISSING;
            if (normal) {
                const double x = pr[a.haploid ? g : gp_src(A, j, k)];
                f = gp_printable(x) ? gp_float_bits(x) : BCF_FLOAT_MISSING;
                if (j++ == k) {
                    ++k;
                    j = 0;
                }
            }
            bcf_put_val(w, at + g * 4, (i32)f, 3);
        }
        return behind;
    }
    // PL: value g of this plane at pos + (lane G + g) width(t); the values of the window alone are written, the whole cell is read to know
    // whether it is all missing
    __device__ __forceinline__ void put_pl(const FmtWindow &w, u64 v, u32 lane, bool mine, u32 t, u64 pos) const
    {
        const u64 w1 = w.w0 + w.wlen;
        const u64 A = a.var_allele_off[v + 1] - a.var_allele_off[v], G = a.haploid ? A : A * (A + 1) / 2;
        if (lane == 0) bcf_put_desc(w, bcf_put_typed_int(w, pos, a.key_pl), (u32)G, t);
        pos += bcf_typed_int_len(a.key_pl) + bcf_desc_len((u32)G);
        const u64 wd = bcf_width(t), at = pos + (u64)lane * G * wd;
        if (!mine || at >= w1 || at + G * wd <= w.w0) return;
        const i32 *pl = a.pl + (u64)lane * a.var_gt_off[a.n_vars] + a.var_gt_off[v];
        bool any = false;
        for (u64 g = 0; g < G && !any; ++g) any = pl[g] != FMT_PL_MISSING;
        const i32 missing = t == 1 ? 0x80 : t == 2 ? 0x8000 : INT32_MIN;
        const u64 g_lo = w.w0 > at ? (w.w0 - at) / wd : 0, g_hi = w1 - at < G * wd ? (w1 - at + wd - 1) / wd : G; // (a value the window cuts is made on both sides)
        for (u64 g = g_lo; g < g_hi; ++g) {
            const i32 x = pl[g];
            bcf_put_val(w, at + g * wd, x != FMT_PL_MISSING ? x : any || g == 0 ? missing : missing + 1, t);
        }
    }
};

template <bool GP, bool PL = false>
__global__ void __launch_bounds__(FMT_TPB) bcf_write_kernel(BcfArgs a, const unsigned char *__restrict__ types, const unsigned long long *__restrict__ row_off,
                                                           char *out, u64 out_cap)
{
    __shared__ __attribute__((aligned(16))) char sh[FMT_WINDOW];
    fmt_write_tile(BcfRows<GP, PL>{a, types}, sh, a.n_vars, row_off, out, out_cap);
}

} // namespace
