// What the host checks of `call` share (tools/call_batch_host_check.cpp, tools/call_worker_host_check.cpp): CHECK, and hand-made records and blocks.
// The including program defines HOST_CHECK_NAME, the name its last line of output starts with.
#pragma once
#include <functional>
#include <iostream>

#include "panel_batch.hpp"

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond "\n";       \
            std::cout << HOST_CHECK_NAME ": FAILED\n";                         \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

template <class T> static bool same(const std::vector<T> &got, std::initializer_list<T> want) { return got == std::vector<T>(want); }
[[maybe_unused]] static bool throws(const std::function<void()> &run)
{
    try {
        run();
    } catch (const std::exception &) {
        return true;
    }
    return false;
}

// a record on `seq`, every kept sample with the genotype g1 g2 (phased or not); its frequencies are 0.5, 0.25, 0.125, ...
static malva::Variant var(const std::string &seq, int pos, const std::string &ref, const std::vector<std::string> &alts, size_t n_samples = 2, int g1 = 0, int g2 = 1,
                          bool phased = true)
{
    malva::Variant v;
    v.seq_name = seq;
    v.ref_pos = pos;
    v.ref_sub = ref;
    v.ref_size = v.min_size = v.max_size = (int)ref.size();
    std::string alt_list;
    for (const auto &a : alts) {
        v.alts.push_back(a);
        v.min_size = std::min(v.min_size, (int)a.size());
        v.max_size = std::max(v.max_size, (int)a.size());
        alt_list += (alt_list.empty() ? "" : ",") + a;
    }
    for (int a = 0; a < v.n_alleles(); ++a) v.frequencies.push_back(std::ldexp(0.5f, -a));
    v.genotypes.assign(n_samples, std::make_pair(g1, g2));
    v.phasing.assign(n_samples, (uint8_t)phased);
    v.text_prefix = seq + "\t" + std::to_string(pos + 1) + "\t.\t" + ref + "\t" + alt_list + "\t.";
    return v;
}
static malva::Block block_of(int k, std::vector<malva::Variant> vars)
{
    malva::Block b(k);
    for (malva::Variant &v : vars) b.add(std::move(v));
    return b;
}

// what a pass hands over, batch by batch
struct Closed {
    std::vector<malva::Rec> recs;
    malva::Batch iso, gen;
};
struct Pass {
    std::vector<Closed> closed;
    std::map<std::string, uint64_t> bases{{"c1", 100}, {"c2", 1100}};
    std::string ref1 = std::string(1000, 'A'), ref2 = std::string(500, 'C');
    std::function<void(std::vector<malva::Rec> &&, malva::Batch &&, malva::Batch &&)> close = [this](std::vector<malva::Rec> &&r, malva::Batch &&i, malva::Batch &&g) {
        closed.push_back({std::move(r), std::move(i), std::move(g)});
    };
    malva::BatchBuilder<decltype(close)> b;
    explicit Pass(const malva::BatchRules &rules) : b(rules, bases, close) {}
    void add(malva::Block blk, const std::string &seq = "c1") { b.add_block(blk, seq, seq == "c2" ? ref2 : ref1); }
};
