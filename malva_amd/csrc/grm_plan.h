// grm_plan.h -- how a step of mg_grm_step is cut into pieces of records (the byte images of a piece fit the scratch cap) and a piece
// into runs along the records, one wave per block of pairs and run, and the constants the cut rests on.  Plain C++, no HIP: the library
// includes it (malva_hip.hip first, then grm_kernels.h for the constants), and tests/test_grm_plan_cpu.py compiles it by itself and
// compares it with its restatement.
//
// The i32 accumulators of grm_gram_kernel rest on `run <= GRM_MAX_RUN` (|h h| <= 2^14 a record: a sum below 2^30).  With one run per
// block the fold needs no atomics (grm_gram_kernel<false>); that happens when the piece is no longer than GRM_MIN_RUN, or when the blocks
// on and above the diagonal alone fill the device and the piece is no longer than GRM_MAX_RUN.
#pragma once
#include <cstdint>

namespace mg {

constexpr uint32_t GRM_K = 64;          // records per MFMA step; a piece's rows are padded to it
constexpr uint32_t GRM_BLOCK = 32;      // a wave's block of pairs: 2 x 2 tiles of 16 x 16
constexpr uint32_t GRM_MAX_RUN = 65536; // records per wave at most (the i32 accumulators), a multiple of GRM_K
constexpr uint64_t GRM_FILL = 2048;     // waves a Gram launch should have (256 CUs x 4 SIMDs x 2): a small cohort is split along the records
constexpr uint64_t GRM_MIN_RUN = 1024;  // ... into runs no shorter than this
static_assert(GRM_MAX_RUN % GRM_K == 0 && GRM_MIN_RUN % GRM_K == 0, "a run of whole MFMA steps may be as long as the longest run");

// the samples padded to whole blocks
inline uint32_t grm_rows(uint32_t n_samples) { return (n_samples + GRM_BLOCK - 1) / GRM_BLOCK * GRM_BLOCK; }

// -> the records of a piece at most: the three byte images (3 bytes per padded sample and record) stay at or under `cap` bytes, unless one
// MFMA step needs more.  A multiple of GRM_K; the last piece of a step is what is left
inline uint64_t grm_piece_max(uint32_t rows, uint64_t cap)
{
    const uint64_t fit = cap / (3ull * rows) / GRM_K * GRM_K;
    return fit > GRM_K ? fit : GRM_K;
}

// a piece's padded row
inline uint64_t grm_ld(uint64_t piece) { return (piece + GRM_K - 1) / GRM_K * GRM_K; }

// -> the records per run (a multiple of GRM_K, at most GRM_MAX_RUN), *n_runs = ceil(ld / run); ld >= GRM_K a multiple of GRM_K, blocks =
// rows / GRM_BLOCK.  Runs: at least ceil(ld / GRM_MAX_RUN); more while the launch has fewer than GRM_FILL waves and a run keeps
// GRM_MIN_RUN records; at most 65,535 (a grid's z)
inline uint64_t grm_run_plan(uint64_t ld, uint32_t blocks, uint64_t *n_runs)
{
    const uint64_t upper = (uint64_t)blocks * (blocks + 1) / 2; // the blocks on and above the diagonal
    const uint64_t steps = ld / GRM_K;
    uint64_t runs = (ld + GRM_MAX_RUN - 1) / GRM_MAX_RUN;
    const uint64_t fill = (GRM_FILL + upper - 1) / upper, keep = (ld + GRM_MIN_RUN - 1) / GRM_MIN_RUN;
    const uint64_t more = fill < keep ? fill : keep;
    if (runs < more) runs = more;
    if (runs > steps) runs = steps;
    if (runs > 65535) runs = 65535;
    const uint64_t run = (steps + runs - 1) / runs * GRM_K; // (at most GRM_MAX_RUN: runs >= ceil(ld / GRM_MAX_RUN), both multiples of GRM_K)
    *n_runs = (ld + run - 1) / run;
    return run;
}

} // namespace mg
