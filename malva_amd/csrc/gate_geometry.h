// gate_geometry.h -- host side of a gate sized in words (BFView::gate_words, kmer_dev.h).  Plain C++, no HIP: the library
// includes it, and tests/test_gate_span_cpu.py compiles it by itself and compares it with its restatement.
#pragma once
#include <cstdint>

namespace mg {

// The geometry of a gate of `words` words (1 <= words <= size / 64) over a filter of `size` bits, as BFView::gate_words describes
// it.  x runs over the top 32 significant bits of the slot range, so xmax = x(size - 1) >= 2^31.  With T = 2^(32 + rs), mul is
// the largest multiplier with xmax * mul < words * T: mul = floor((words * T - 1) / xmax), and rs the largest shift at which
// it still fits 32 bits (a multiplier of few bits cuts a gate of few words unevenly: at rs = 0, 24 words over 2^18 + 77 slots
// get a multiplier of 47 where 47.99 is wanted, and the last word is half empty).  Then x * mul / T <= words - 1 for every slot,
// and xmax * (mul + 1) >= words * T gives xmax * mul >= words * T - xmax > (words - 1) * T: the last slot lands in the last word.
inline void gate_geometry(uint64_t size, uint64_t words, uint32_t *mul, uint32_t *ls, uint32_t *rs, uint32_t *mask_shift)
{
    uint32_t L = 1;
    while (L < 64 && ((size - 1) >> L)) ++L;
    *ls = 64 - L;
    const uint64_t xmax = ((size - 1) << *ls) >> 32;
    *mul = *rs = 0;
    for (uint32_t e = 0; xmax && e < 32; ++e) { // (xmax = 0: a filter of one bit)
        const unsigned __int128 m = ((((unsigned __int128)words) << (32 + e)) - 1) / xmax;
        if (m > 0xFFFFFFFFULL) break;
        *mul = (uint32_t)m;
        *rs = e;
    }
    uint32_t g = 6; // 2^g <= size / words < 2^(g+1): the slots of one word differ in their low g bits
    while (g < 63 && (size / words) >> (g + 1)) ++g;
    *mask_shift = g - 6;
}
// the word of slot idx, as the device computes it (kmer_dev.h, gate_word)
inline uint64_t gate_word_of(uint64_t idx, uint32_t mul, uint32_t ls, uint32_t rs)
{
    return (((uint64_t)(uint32_t)((idx << ls) >> 32) * mul) >> 32) >> rs;
}

} // namespace mg
