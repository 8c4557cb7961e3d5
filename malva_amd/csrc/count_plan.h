// count_plan.h -- how the word axis of mg_pair_counts and the record axis of mg_sample_counts are cut into runs, one workgroup per
// run, and the constants the cut rests on.  Plain C++, no HIP: the library includes it (malva_hip.hip first, then pair_kernels.h and
// sample_kernels.h for the constants), and tests/test_count_plan_cpu.py compiles it by itself and compares it with its restatement.
//
// Both plans are one rule: the axis of n units in whole chunks, as many runs as give about `target` workgroups over all `div` tiles or
// planes -- but at least enough that no run is longer than `max_run`, on which the 32-bit partial sums of the two kernels rest (a sum
// below 2^26 in pair_kernels.h, an accumulator below 2^19 in sample_kernels.h).  max_run is a multiple of chunk, so rounding a run up to
// whole chunks cannot take it past max_run: with runs >= ceil(n / max_run), ceil(chunks / runs) <= max_run / chunk.
#pragma once
#include <cstdint>

namespace mg {

constexpr uint32_t PAIR_CHUNK = 32;           // words of every plane staged at a time
constexpr uint64_t PAIR_MAX_RUN = 1u << 20;   // words per workgroup at most (the 32-bit sums), a multiple of PAIR_CHUNK
constexpr uint64_t PAIR_TARGET_WGS = 2048;
constexpr uint32_t SAMPLE_TPB = 256;          // four waves, 256 consecutive records of one plane per step
constexpr uint64_t SAMPLE_MAX_RUN = 1u << 20; // records per workgroup at most (the 32-bit accumulators), a multiple of SAMPLE_TPB
constexpr uint64_t SAMPLE_TARGET_WGS = 2048;
static_assert(PAIR_MAX_RUN % PAIR_CHUNK == 0 && SAMPLE_MAX_RUN % SAMPLE_TPB == 0, "a run of whole chunks may be as long as the longest run");

// -> the units per run (a multiple of chunk), *n_runs = ceil(n / run); n >= 1, div >= 1
inline uint64_t count_plan(uint64_t n, uint32_t div, uint64_t chunk, uint64_t target, uint64_t max_run, uint64_t *n_runs)
{
    const uint64_t chunks = (n + chunk - 1) / chunk;
    const uint64_t wanted = target / div > 1 ? target / div : 1;
    uint64_t runs = chunks < wanted ? chunks : wanted;
    const uint64_t least = (n + max_run - 1) / max_run;
    if (runs < least) runs = least;
    const uint64_t run = (chunks + runs - 1) / runs * chunk; // (whole chunks; at most max_run, itself a multiple of chunk)
    *n_runs = (n + run - 1) / run;
    return run;
}

// The word axis is cut into runs, one workgroup per tile of pairs and run: as many runs as give about PAIR_TARGET_WGS workgroups -- with
// one tile (2 planes x 1e7 records) all the parallelism comes from here --, none longer than PAIR_MAX_RUN (the 32-bit sums)
inline uint64_t pair_count_plan(uint64_t n_words, uint32_t tiles, uint64_t *n_runs)
{
    return count_plan(n_words, tiles, PAIR_CHUNK, PAIR_TARGET_WGS, PAIR_MAX_RUN, n_runs);
}

// The records are cut into runs, one workgroup per plane and run: as many runs as give about SAMPLE_TARGET_WGS workgroups over all
// planes -- a chip's worth of waves, and a few dozen atomic adds per counter --, none longer than SAMPLE_MAX_RUN (the 32-bit accumulators)
inline uint64_t sample_count_plan(uint64_t n_vars, uint32_t n_planes, uint64_t *n_runs)
{
    return count_plan(n_vars, n_planes, SAMPLE_TPB, SAMPLE_TARGET_WGS, SAMPLE_MAX_RUN, n_runs);
}

} // namespace mg
