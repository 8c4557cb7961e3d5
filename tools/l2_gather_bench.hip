// Microbenchmark behind DESIGN.md's bound for the scan's filter kernel: how many independent, uniformly random
// 8-byte reads per second one MI355X sustains from a table of F bytes (F = 16 KiB .. 1 GiB: L2-resident up to
// 4 MiB per XCD), alone and beside a non-temporal 20-byte-per-lane stream shaped like the k-mer table.  Then the same for tables
// of 1..8 MiB whose word count is no power of two, beside the 20 B/row stream and beside the packed 12 B/row one
// (profiles/gate_span_l2_gather.txt: flat up to 3 MiB, +0.02 ms at 3.5 MiB, +0.06 ms at 4 MiB).
//   make microbench && bin/l2_gather_bench
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e = (x);                                                                    \
        if (e != hipSuccess) {                                                                 \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));                             \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

// rows: n; every thread takes 2 rows per iteration (as the filter kernel), reads the stream (optional) and one
// random word of the table per row; the word index is a cheap mix of the row number (or of the streamed data)
// SPOL: cache policy of the stream's loads (buffer builtins' aux: 1 sc0, 2 nt, 16 sc1), -1 = flat nt loads
template <bool STREAM, bool GATHER, int SPOL = -1>
__global__ void __launch_bounds__(256) bench(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo,
                                             const uint32_t *__restrict__ cnt, uint64_t n, const uint64_t *__restrict__ table,
                                             uint64_t mask, unsigned long long *sink)
{
    uint64_t acc = 0;
    const uint64_t step = (uint64_t)gridDim.x * 512;
    for (uint64_t base = (uint64_t)blockIdx.x * 512; base + 512 <= n; base += step) {
        const uint64_t i = base + 2 * threadIdx.x;
        uint64_t a0 = i * 0x9E3779B97F4A7C15ULL, a1 = (i + 1) * 0x9E3779B97F4A7C15ULL;
        if (STREAM && SPOL >= 0) {
            typedef unsigned int __attribute__((ext_vector_type(4))) v4u;
            typedef unsigned int __attribute__((ext_vector_type(2))) v2u;
            const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc((void *)lo, 0, 0x7FFFFFFF, 0x00020000);
            const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void *)hi, 0, 0x7FFFFFFF, 0x00020000);
            const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void *)cnt, 0, 0x7FFFFFFF, 0x00020000);
            const v4u l4 = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)(i * 8), 0, SPOL);
            const v4u h4 = __builtin_amdgcn_raw_buffer_load_b128(rh, (int)(i * 8), 0, SPOL);
            const v2u c2 = __builtin_amdgcn_raw_buffer_load_b64(rc, (int)(i * 4), 0, SPOL);
            a0 ^= l4.x + h4.y + c2.x + ((uint64_t)(l4.y ^ h4.x) << 32);
            a1 ^= l4.z + h4.w + c2.y + ((uint64_t)(l4.w ^ h4.z) << 32);
        } else if (STREAM) {
            typedef unsigned long long __attribute__((ext_vector_type(2))) v2u64;
            typedef unsigned int __attribute__((ext_vector_type(2))) v2u32;
            const v2u64 l2 = __builtin_nontemporal_load((const v2u64 *)(lo + i));
            const v2u64 h2 = __builtin_nontemporal_load((const v2u64 *)(hi + i));
            const v2u32 c2 = __builtin_nontemporal_load((const v2u32 *)(cnt + i));
            a0 ^= l2.x + h2.x + c2.x;
            a1 ^= l2.y + h2.y + c2.y;
        }
        a0 ^= a0 >> 29;
        a1 ^= a1 >> 29;
        a0 *= 0xBF58476D1CE4E5B9ULL;
        a1 *= 0xBF58476D1CE4E5B9ULL;
        if (GATHER) {
            const uint64_t g0 = table[(a0 >> 20) & mask], g1 = table[(a1 >> 20) & mask];
            acc += g0 + g1;
        } else
            acc += a0 + a1;
    }
    if (acc == 0x1234567) atomicAdd(sink, 1ULL);
}

// The same beside a table whose word count is no power of two (a gate of 2..4 MiB that leaves the stream room in L2): the word
// index is a multiply-high of 32 mixed bits, as BFView::gate_words scales a filter slot.  ROWB: bytes per row of the stream,
// 20 (the SoA table, as above) or 12 (packed rows: three 8-byte loads per thread, as scan_filter12_kernel), 0 = no stream.
template <int ROWB>
__global__ void __launch_bounds__(256) bench_span(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo,
                                                  const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ rows12, uint64_t n,
                                                  const uint64_t *__restrict__ table, uint32_t words, unsigned long long *sink)
{
    uint64_t acc = 0;
    const uint64_t step = (uint64_t)gridDim.x * 512;
    for (uint64_t base = (uint64_t)blockIdx.x * 512; base + 512 <= n; base += step) {
        const uint64_t i = base + 2 * threadIdx.x;
        uint64_t a0 = i * 0x9E3779B97F4A7C15ULL, a1 = (i + 1) * 0x9E3779B97F4A7C15ULL;
        typedef unsigned long long __attribute__((ext_vector_type(2))) v2u64;
        typedef unsigned int __attribute__((ext_vector_type(2))) v2u32;
        if (ROWB == 20) {
            const v2u64 l2 = __builtin_nontemporal_load((const v2u64 *)(lo + i));
            const v2u64 h2 = __builtin_nontemporal_load((const v2u64 *)(hi + i));
            const v2u32 c2 = __builtin_nontemporal_load((const v2u32 *)(cnt + i));
            a0 ^= l2.x + h2.x + c2.x;
            a1 ^= l2.y + h2.y + c2.y;
        } else if (ROWB == 12) {
            const v2u32 *src = (const v2u32 *)rows12 + 3 * (i / 2);
            const v2u32 w0 = __builtin_nontemporal_load(src), w1 = __builtin_nontemporal_load(src + 1), w2 = __builtin_nontemporal_load(src + 2);
            a0 ^= w0.x + ((uint64_t)w0.y << 32) + w1.x;
            a1 ^= w1.y + ((uint64_t)w2.x << 32) + w2.y;
        }
        a0 ^= a0 >> 29;
        a1 ^= a1 >> 29;
        a0 *= 0xBF58476D1CE4E5B9ULL;
        a1 *= 0xBF58476D1CE4E5B9ULL;
        acc += table[__umulhi((uint32_t)(a0 >> 20), words)] + table[__umulhi((uint32_t)(a1 >> 20), words)];
    }
    if (acc == 0x1234567) atomicAdd(sink, 1ULL);
}

int main()
{
    const uint64_t n = 100000000ULL / 512 * 512;
    uint64_t *hi, *lo, *table;
    uint32_t *cnt;
    unsigned long long *sink;
    CK(hipMalloc(&hi, n * 8));
    CK(hipMalloc(&lo, n * 8));
    CK(hipMalloc(&cnt, n * 4));
    CK(hipMalloc(&table, 1ULL << 30));
    CK(hipMalloc(&sink, 8));
    CK(hipMemset(hi, 1, n * 8));
    CK(hipMemset(lo, 2, n * 8));
    CK(hipMemset(cnt, 3, n * 4));
    CK(hipMemset(table, 5, 1ULL << 30));
    CK(hipMemset(sink, 0, 8));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto time = [&](auto kern, uint64_t mask) -> float {
        float best = 1e9f;
        for (int rep = 0; rep < 6; ++rep) {
            hipEventRecord(e0, 0);
            hipLaunchKernelGGL(kern, dim3(8192), dim3(256), 0, 0, hi, lo, cnt, n, table, mask, sink);
            hipEventRecord(e1, 0);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            if (rep && ms < best) best = ms;
        }
        return best;
    };
    printf("rows %llu, 2 rows per thread, grid 8192 x 256\n", (unsigned long long)n);
    const float s_only = time(bench<true, false>, 0);
    printf("stream only (20 B/row, nt):            %.3f ms  %.2f TB/s\n", s_only, n * 20.0 / s_only * 1e-9);
    const float none = time(bench<false, false>, 0);
    printf("no memory (index arithmetic only):      %.3f ms\n", none);
    {
        const uint64_t m4 = (4ULL << 20) / 8 - 1;
        printf("stream policy, alone / beside a 4 MiB gather:  flat nt %.3f / %.3f | buffer plain %.3f / %.3f | sc0 %.3f / %.3f | nt %.3f / %.3f | sc1 %.3f / %.3f |"
               " sc0 sc1 %.3f / %.3f | sc1 nt %.3f / %.3f | sc0 sc1 nt %.3f / %.3f ms\n",
               time(bench<true, false>, 0), time(bench<true, true>, m4), time(bench<true, false, 0>, 0), time(bench<true, true, 0>, m4),
               time(bench<true, false, 1>, 0), time(bench<true, true, 1>, m4), time(bench<true, false, 2>, 0), time(bench<true, true, 2>, m4),
               time(bench<true, false, 16>, 0), time(bench<true, true, 16>, m4), time(bench<true, false, 17>, 0), time(bench<true, true, 17>, m4),
               time(bench<true, false, 18>, 0), time(bench<true, true, 18>, m4), time(bench<true, false, 19>, 0), time(bench<true, true, 19>, m4));
    }
    for (int lg = 14; lg <= 30; lg += (lg < 26 ? 2 : 1)) {
        const uint64_t words = (1ULL << lg) / 8;
        const float g = time(bench<false, true>, words - 1), sg = time(bench<true, true>, words - 1);
        printf("table %6llu KiB: gather only %.3f ms = %.3g reads/s | stream + gather %.3f ms = %.3g rows/s (stream only + gather only = %.3f)\n",
               (unsigned long long)((1ULL << lg) >> 10), g, n / (g * 1e-3), sg, n / (sg * 1e-3), s_only + g);
    }
    // between 1 MiB and 4 MiB: does a table that leaves the stream room in an XCD's 4 MiB L2 gather faster beside it?
    uint32_t *rows12;
    CK(hipMalloc(&rows12, n * 12));
    CK(hipMemset(rows12, 4, n * 12));
    auto time_span = [&](auto kern, uint32_t words) -> float {
        float best = 1e9f;
        for (int rep = 0; rep < 6; ++rep) {
            hipEventRecord(e0, 0);
            hipLaunchKernelGGL(kern, dim3(8192), dim3(256), 0, 0, hi, lo, cnt, rows12, n, table, words, sink);
            hipEventRecord(e1, 0);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            if (rep && ms < best) best = ms;
        }
        return best;
    };
    printf("word index by multiply-high (any table size):\n");
    for (int kib : {1024, 2048, 2560, 3072, 3584, 4096, 8192}) {
        const uint32_t words = (uint32_t)kib * 128u;
        const float g = time_span(bench_span<0>, words), s20 = time_span(bench_span<20>, words), s12 = time_span(bench_span<12>, words);
        printf("table %6d KiB: gather only %.3f ms | 20 B/row stream + gather %.3f ms | 12 B/row stream + gather %.3f ms\n", kib, g, s20, s12);
    }
    CK(hipGetLastError());
    return 0;
}
