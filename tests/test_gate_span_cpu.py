"""The gate sized in words (BFView::gate_words, csrc/kmer_dev.h): the slot -> word mapping and the mask's inputs, restated in
Python from the device code and the host's gate_geometry (csrc/gate_geometry.h) and checked at the edges of the slot range; the
header itself is compiled on the host and held against the restatement.

    x    = high dword of (idx << ls),           ls = 64 - bit length of (size - 1)
    word = x * mul >> (32 + rs),                mul = floor((words * 2^(32 + rs) - 1) / x(size - 1)), rs the largest with mul < 2^32
    mask = gate_mask_sk(idx, g - 6, k),         2^g <= size / words < 2^(g+1)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

M64 = (1 << 64) - 1
SIZES = [1 << 17, 1 << 33, (1 << 18) + 77]
WORDS = [1, 3, 5 * 2 ** 3, 3 * 2 ** 17]


def geometry(size, words):
    L = max(1, (size - 1).bit_length())
    ls = 64 - L
    xmax = (((size - 1) << ls) & M64) >> 32
    rs = max(e for e in range(32) if ((words << (32 + e)) - 1) // xmax <= 0xFFFFFFFF)
    mul = ((words << (32 + rs)) - 1) // xmax
    g = max(6, (size // words).bit_length() - 1)
    return (mul, ls, rs), g - 6


def gate_word(idx, geo):
    mul, ls, rs = geo
    return (((((idx << ls) & M64) >> 32) * mul) >> 32) >> rs


def gate_words_np(idx, geo):
    mul, ls, rs = geo
    x = (idx << np.uint64(ls)) >> np.uint64(32)                            # uint64 arithmetic wraps as the device's does
    return ((x * np.uint64(mul)) >> np.uint64(32)) >> np.uint64(rs)        # x, mul < 2^32: the product fits


def gate_mask(idx, shift, k=4):
    m = 1 << ((idx >> shift) & 63)
    t = idx & ((1 << min(shift + 6, 24)) - 1)
    for c in (0x9E3779, 0xEBCA77, 0xB2AE3D)[:k - 1]:
        m |= 1 << ((((t & 0xFFFFFF) * c) & 0xFFFFFFFF) >> 26)
    return m


SHIM = r"""
#include "gate_geometry.h"
extern "C" void geometry(uint64_t size, uint64_t words, uint32_t *out) { mg::gate_geometry(size, words, out, out + 1, out + 2, out + 3); }
extern "C" void words_of(const uint64_t *idx, uint64_t n, uint32_t mul, uint32_t ls, uint32_t rs, uint64_t *out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = mg::gate_word_of(idx[i], mul, ls, rs);
}
"""


@pytest.fixture(scope="module")
def host_geometry(tmp_path_factory):
    """the library's own gate_geometry (csrc/gate_geometry.h, plain C++), compiled by itself"""
    d = tmp_path_factory.mktemp("gate_geometry")
    src, so = d / "shim.cpp", d / "libgate_geometry.so"
    src.write_text(SHIM)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", "-I", os.path.join(root, "malva_amd", "csrc"), "-o", str(so), str(src)],
                   check=True, capture_output=True)
    return ctypes.CDLL(str(so))


@pytest.mark.parametrize("size", SIZES + [64, 65, 1000003, (1 << 35), (1 << 37) - 3])
@pytest.mark.parametrize("words", WORDS + [2, 24, 2048, 3072 * 128])
def test_host_geometry_is_the_restatement(host_geometry, size, words):
    """what alloc_gate puts into the view equals what the tests above reason about, and its words stay inside the gate"""
    words = min(words, max(1, size // 64))                 # as alloc_gate clamps it (gate_words_max)
    out = (ctypes.c_uint32 * 4)()
    host_geometry.geometry(ctypes.c_uint64(size), ctypes.c_uint64(words), out)
    (mul, ls, rs), shift = geometry(size, words)
    assert (out[0], out[1], out[2], out[3]) == (mul, ls, rs, shift)
    rng = np.random.default_rng(size % 977 + words)
    idx = np.concatenate([rng.integers(0, size, size=20_000, dtype=np.uint64), np.array([0, size - 1], dtype=np.uint64)])
    got = np.zeros(idx.size, dtype=np.uint64)
    host_geometry.words_of(idx.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(idx.size), ctypes.c_uint32(mul), ctypes.c_uint32(ls),
                           ctypes.c_uint32(rs), got.ctypes.data_as(ctypes.c_void_p))
    assert np.array_equal(got, gate_words_np(idx, (mul, ls, rs)))
    assert int(got.max()) == words - 1 and int(got[-2]) == 0


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("words", WORDS)
def test_first_and_last_slot_and_nothing_beyond(size, words):
    geo, _ = geometry(size, words)
    assert 0 < geo[0] <= 0xFFFFFFFF and 0 <= geo[2] < 32
    assert gate_word(0, geo) == 0
    assert gate_word(size - 1, geo) == words - 1
    rng = np.random.default_rng(size % 1000 + words)
    idx = rng.integers(0, size, size=100_000, dtype=np.uint64)
    edge = np.array([0, 1, size // 2, size - 2, size - 1], dtype=np.uint64)
    idx = np.sort(np.concatenate([idx, edge]))
    w = gate_words_np(idx, geo)
    assert int(w.max()) == words - 1 and int(w.min()) == 0
    assert np.all(np.diff(w.astype(np.int64)) >= 0)        # words lie in the order of the slots: contiguous runs
    for i in (0, 1, size - 1, int(idx[12345])):            # the vector form is the scalar one
        assert gate_word(i, geo) == int(gate_words_np(np.array([i], dtype=np.uint64), geo)[0])


@pytest.mark.parametrize("size", SIZES)
def test_every_word_of_a_24_word_gate_is_hit_evenly(size):
    geo, _ = geometry(size, 24)
    idx = np.random.default_rng(24).integers(0, size, size=100_000, dtype=np.uint64)
    fill = np.bincount(gate_words_np(idx, geo).astype(np.int64), minlength=24)
    assert len(fill) == 24 and fill.min() > 0
    assert fill.max() <= 2 * fill.min()


# (a word of 3 * 2^17 words over 2^17 or 2^18 + 77 slots holds at most one slot: no pairs to compare there)
@pytest.mark.parametrize("size,words", [(s, w) for s in SIZES for w in WORDS if s // w >= 4])
def test_slots_of_one_word_that_differ_in_low_bits_get_different_masks(size, words):
    """The mask's inputs are bits in which two slots of one word can differ: the six bits below the word's span for the first
    position, the low min(g, 24) bits for the others.  Pairs that share a word and differ only there get different masks in
    more than 9 cases of 10 (identical masks make the extra bits worthless: the 5.6 % incident noted at gate_mask_sk)."""
    geo, shift = geometry(size, words)
    low = min(shift + 6, 24)
    rng = np.random.default_rng(7)
    a = rng.integers(0, size, size=20_000, dtype=np.uint64)
    b = a ^ rng.integers(1, 1 << low, size=a.size, dtype=np.uint64)
    keep = (b < size) & (gate_words_np(a, geo) == gate_words_np(np.minimum(b, np.uint64(size - 1)), geo))
    a, b = a[keep][:5000], b[keep][:5000]
    assert a.size > 2_000
    differ = sum(gate_mask(int(x), shift) != gate_mask(int(y), shift) for x, y in zip(a, b))
    assert differ > 0.9 * a.size
    # and every position of the mask is in use: over many slots all 64 bits of a word get set
    union = 0
    for x in a:
        union |= gate_mask(int(x), shift)
    assert union == M64
