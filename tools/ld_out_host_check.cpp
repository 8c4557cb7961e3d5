// The host half of `call --cohort --ld` (malva_amd/host/cohort_out.hpp) driven without a device: the table's text on hand-written pairs, the
// groups' word streams written and read back across 1, 2 and 3 groups with a made-up window function in the device's place -- chunk sizes that put
// window, chunk and contig boundaries in every relative position, a window larger than a chunk, a buffer that has to grow --, streams cut short, too
// long or mismatched, and the PATH.part hand-over.  Meant to be built with -fsanitize=address,undefined and run on the CPU (`make sanitize-host`);
// tests/test_ld_out_cpu.py builds it plain.  It takes a scratch directory as its argument and exits non-zero on the first wrong answer.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>

#include "cohort_out.hpp"

using namespace malva;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond "\n";       \
            std::cout << "ld_out_host_check: FAILED\n";                        \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static bool exists(const std::string &p) { return access(p.c_str(), F_OK) == 0; }
static std::string slurp(const std::string &p)
{
    std::ifstream in(p, std::ios::binary);
    std::stringstream all;
    all << in.rdbuf();
    return all.str();
}
static std::string error_of(const std::function<void()> &run)
{
    try {
        run();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return std::string();
}
static bool has(const std::string &text, const char *piece) { return text.find(piece) != std::string::npos; }

// In the device's place: a pair is emitted when it is eligible as mg_ld_window says and some sample of some group has a bit in both records; its
// values show every input and print exactly.  The buffer contract is the library's.
struct Fake {
    size_t window;
    uint64_t max_bp;
    size_t calls = 0, limits = 0, most_vars = 0;
    int operator()(size_t n_vars, size_t n_first, size_t G, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, mg_ld_pair *pairs, size_t cap, uint64_t *row_off,
                   uint64_t *needed)
    {
        ++calls;
        most_vars = std::max(most_vars, n_vars);
        CHECK(n_first <= n_vars && G >= 1);
        uint64_t k = 0;
        for (size_t i = 0; i < n_first; ++i) {
            row_off[i] = k;
            for (size_t j = i + 1; j <= i + window && j < n_vars; ++j) {
                const long long d = (long long)pos[j] - (long long)pos[i];
                if (chrom[i] != chrom[j] || (max_bp && (uint64_t)(d < 0 ? -d : d) > max_bp)) continue;
                uint32_t n = 0;
                for (size_t g = 0; g < G; ++g) {
                    const uint64_t *s = sites + g * 3 * n_vars;
                    n += (uint32_t)__builtin_popcountll((s[i] | s[n_vars + i] | s[2 * n_vars + i]) & (s[j] | s[n_vars + j] | s[2 * n_vars + j]));
                }
                if (!n) continue;
                if (k < cap) pairs[k] = mg_ld_pair{(uint32_t)i, (uint32_t)j, n, (int32_t)(n % 3) - 1, (double)n / 1024.0 + (double)(j - i) / 8.0};
                ++k;
            }
        }
        row_off[n_first] = k;
        *needed = k;
        if (k > cap) ++limits;
        return k > cap ? MG_ERR_LIMIT : MG_OK;
    }
};

struct Record {
    std::string cols;
    uint32_t A;
    std::vector<uint64_t> words; // [groups][3]
};

static void text_rules()
{
    std::string out;
    const std::string a = "c1\t7\trs1", b = "c1\t19\t.";
    ld_row(out, a, b, 3, mg_ld_pair{0, 1, 12, 1, 0.25});
    ld_row(out, a, b, 3, mg_ld_pair{0, 1, 16384, -1, 1.0 / 3.0});
    ld_row(out, a, b, 3, mg_ld_pair{0, 1, 2, 0, 0.0});
    ld_row(out, a, b, 3, mg_ld_pair{0, 1, 2, 1, 1e-7});
    CHECK(out == "c1\t7\trs1\t19\t.\t12\t0.25\t+\n" "c1\t7\trs1\t19\t.\t16384\t0.333333\t-\n" "c1\t7\trs1\t19\t.\t2\t0\t0\n" "c1\t7\trs1\t19\t.\t2\t1e-07\t+\n");
    CHECK(std::string(ld_header()) == "#CHROM\tPOS_A\tID_A\tPOS_B\tID_B\tN\tR2\tSIGN\n");
    std::string s;
    put_site_words(s, 1, 2, 3, 2, nullptr, 0);
    CHECK(s.size() == 28);
    put_site_words(s, 1, 2, 3, 2, "abc", 3);
    CHECK(s.size() == 28 + 28 + 4 + 3);
}

// n records on four contigs (the third a single record), positions 10 apart with a few long gaps; record v % 7 == 3 has no bit anywhere
static std::vector<Record> records(size_t n, size_t groups)
{
    std::vector<Record> recs;
    uint32_t pos = 100;
    for (size_t v = 0; v < n; ++v) {
        Record r;
        const size_t contig = v < n / 3 ? 0 : v == n / 3 ? 1 : v < 2 * n / 3 ? 2 : 3;
        if (v && (v == n / 3 || v == n / 3 + 1 || v == 2 * n / 3)) pos = 50;
        pos += v % 5 == 4 ? 400 : 10;
        r.A = v % 7 == 3 ? 3 : 2;
        r.cols = "chr" + std::to_string(contig) + "\t" + std::to_string(pos) + "\t" + (v % 4 ? "id" + std::to_string(v) : ".") + "\tA\t" + (r.A == 3 ? "C,G" : "C");
        for (size_t g = 0; g < groups; ++g)
            for (uint64_t d = 0; d < 3; ++d) r.words.push_back(r.A == 2 ? (0x9E3779B97F4A7C15ull * (v + 1) >> (7 * g + 3 * d)) & (0x249249ull << d) & ((1ull << (5 + 9 * g)) - 1) : 0ull);
        recs.push_back(r);
    }
    return recs;
}
static std::vector<std::string> streams(const std::vector<Record> &recs, size_t groups)
{
    std::vector<std::string> out(groups);
    for (const Record &r : recs)
        for (size_t g = 0; g < groups; ++g) put_site_words(out[g], r.words[3 * g], r.words[3 * g + 1], r.words[3 * g + 2], r.A, g ? nullptr : r.cols.data(), r.cols.size());
    return out;
}
// the whole table in one call, without the reader
static std::string expected(const std::vector<Record> &recs, size_t groups, Fake fake)
{
    const size_t n = recs.size();
    std::vector<uint64_t> sites(3 * groups * n), row_off(n + 1);
    std::vector<uint32_t> chrom(n), pos(n);
    std::vector<std::string> cols(n);
    std::vector<size_t> pos_at(n);
    for (size_t v = 0; v < n; ++v) {
        for (size_t k = 0; k < 3 * groups; ++k) sites[k * n + v] = recs[v].words[k];
        const std::string &c = recs[v].cols;
        const size_t t0 = c.find('\t'), t1 = c.find('\t', t0 + 1), t2 = c.find('\t', t1 + 1);
        chrom[v] = (uint32_t)atoi(c.c_str() + 3);
        pos[v] = (uint32_t)atoi(c.c_str() + t0 + 1);
        cols[v] = c.substr(0, t2);
        pos_at[v] = t0 + 1;
    }
    std::vector<mg_ld_pair> pairs(n * fake.window + 1);
    uint64_t needed = 0;
    CHECK(fake(n, n, groups, sites.data(), chrom.data(), pos.data(), pairs.data(), pairs.size(), row_off.data(), &needed) == MG_OK);
    std::string out = ld_header();
    for (uint64_t k = 0; k < needed; ++k) ld_row(out, cols[pairs[k].i], cols[pairs[k].j], pos_at[pairs[k].j], pairs[k]);
    return out;
}
static void fill(std::deque<PartFile> &files, const std::string &base, const std::vector<std::string> &contents)
{
    for (size_t g = 0; g < contents.size(); ++g) {
        files.emplace_back();
        files.back().open(base + ".g" + std::to_string(g) + ".sites.part", PartFile::SCRATCH);
        files.back().write(contents[g]);
        files.back().finish();
    }
}
// the pass as the driver runs it: the table through a PartFile, the groups' streams gone before it takes its name
static std::string run_pass(const std::string &dir, const std::vector<std::string> &contents, size_t chunk, Fake &fake)
{
    const std::string path = dir + "/ld.tsv";
    {
        std::deque<PartFile> files;
        PartFile table;
        fill(files, path, contents);
        table.open(path);
        ld_table(files, fake.window, chunk, fake, [&](const char *data, size_t n) { table.write(data, n); });
        CHECK(!exists(path) && exists(path + ".part"));
        files.clear();
        table.finish();
    }
    CHECK(exists(path) && !exists(path + ".part"));
    for (size_t g = 0; g < contents.size(); ++g) CHECK(!exists(path + ".g" + std::to_string(g) + ".sites.part"));
    const std::string text = slurp(path);
    unlink(path.c_str());
    return text;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::cerr << "usage: ld_out_host_check SCRATCH_DIR\n";
        return 2;
    }
    const std::string dir = argv[1];
    text_rules();
    for (size_t groups = 1; groups <= 3; ++groups) {
        const std::vector<Record> recs = records(41, groups);
        const std::vector<std::string> contents = streams(recs, groups);
        size_t lines_seen = 0;
        for (size_t window : {(size_t)1, (size_t)2, (size_t)3, (size_t)8, (size_t)50})
            for (uint64_t max_bp : {(uint64_t)0, (uint64_t)35}) {
                const std::string want = expected(recs, groups, Fake{window, max_bp});
                lines_seen = std::max<size_t>(lines_seen, std::count(want.begin(), want.end(), '\n'));
                for (size_t chunk = 1; chunk <= 45; chunk += chunk < 16 ? 1 : 13) { // every chunk size up to 16 (a window of 8 and contigs of 13 in every position), then 29 and 42 (the whole table)
                    Fake fake{window, max_bp};
                    CHECK(run_pass(dir, contents, chunk, fake) == want);
                    CHECK(fake.most_vars <= chunk + window && fake.limits == 0);
                    CHECK(fake.calls == 1 + (41 >= window ? (41 - window) / chunk : 0)); // (a chunk leaves while chunk + window records are in hand; the look-ahead records are the head of the next)
                }
            }
        CHECK(lines_seen > 100);
        {   // no record at all: the header alone
            Fake fake{8, 0};
            CHECK(run_pass(dir, std::vector<std::string>(groups), 5, fake) == ld_header() && fake.calls == 0);
        }
        {   // more pairs in a chunk than the first buffer holds: MG_ERR_LIMIT once, then the buffer asked for
            const std::vector<Record> many = records(300, groups);
            Fake fake{50, 0};
            const std::string want = expected(many, groups, fake);
            CHECK(std::count(want.begin(), want.end(), '\n') > 3000);
            CHECK(run_pass(dir, streams(many, groups), 250, fake) == want);
            CHECK(fake.limits == 1 && fake.calls == 3);
        }

        // streams cut short, longer than the first, or of another record: an error, the table never under its name, nothing left
        const std::string path = dir + "/ld.tsv";
        auto failing = [&](std::vector<std::string> bad, const char *why_piece) {
            const std::string why = error_of([&] {
                std::deque<PartFile> files;
                PartFile table;
                fill(files, path, bad);
                table.open(path);
                Fake fake{3, 0};
                ld_table(files, 3, 4, fake, [&](const char *data, size_t n) { table.write(data, n); });
                table.finish();
            });
            CHECK(has(why, why_piece));
            CHECK(!exists(path) && !exists(path + ".part") && !exists(path + ".g0.sites.part"));
        };
        for (size_t g = 0; g < groups; ++g) {
            std::vector<std::string> bad = contents;
            bad[g].resize(bad[g].size() - 3);
            failing(bad, "LD table are short");
            if (!g) continue; // (the first stream cut at a record's end is a shorter panel, not an error of its own)
            bad = contents;
            bad[g].resize(bad[g].size() / 2);
            failing(bad, "LD table are short");
        }
        if (groups > 1) {
            std::vector<std::string> bad = contents;
            bad[groups - 1] += bad[groups - 1]; // more records than the first group has
            failing(bad, "LD table are short");
            bad = contents;
            uint32_t other = 5;
            memcpy(&bad[1][24], &other, 4); // a record with another number of alleles
            failing(bad, "LD table are short");
        }
        std::vector<std::string> bad = contents;
        bad[0].replace(32, 4, "chrX"); // (the first record's columns start behind 24 + 4 + 4 bytes) columns without a tab
        const uint32_t len = 4;
        bad[0].replace(28, 4, (const char *)&len, 4);
        bad[0].erase(36, recs[0].cols.size() - 4);
        failing(bad, "columns in the LD table's stream are short");
    }
    std::cout << "ld_out_host_check: ok\n";
    return 0;
}
