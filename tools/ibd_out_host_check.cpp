// The host half of `call --cohort --ibd` (malva_amd/host/cohort_out.hpp) driven without a device: the table's text on hand-written segments, the
// groups' word streams written and read back under several groupings of the same cohort -- groups of 64 + 6, 35 + 35, 10 + 20 + 40 and seventy of one
// sample, whose words have to land in the same cohort-wide bits -- with the definition's own loop on the CPU in the device's place, chunk sizes from one
// record to the whole table, a buffer that has to grow (the refused step must not move the state), a cohort of one sample, streams cut short, and the
// PATH.part hand-over.  Every grouping and chunk size must give the same bytes.  Meant to be built with -fsanitize=address,undefined and run on the
// CPU (`make sanitize-host`); tests/test_ibd_out_cpu.py builds it plain.  It takes a scratch directory as its argument and exits non-zero on the first
// wrong answer.
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
            std::cout << "ibd_out_host_check: FAILED\n";                       \
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

// In the device's place: mg_ibd_begin's state and mg_ibd_step's walk, record by record as the definition says.  The buffer contract is the
// library's: a step that does not fit reports its need and leaves the state where it was.
struct Pair {
    bool open = false;
    uint32_t chrom = 0, start = 0, end = 0, n = 0, ibs2 = 0;
};
struct Fake {
    size_t S;
    uint32_t min_records;
    long long min_bp;
    std::vector<Pair> state;
    size_t calls = 0, limits = 0, most_vars = 0, flushes = 0;
    Fake(size_t S, uint32_t min_records, long long min_bp) : S(S), min_records(min_records), min_bp(min_bp), state(S * (S - 1) / 2) {}
    static int dosage(const uint64_t *sites, size_t n_vars, size_t v, size_t s)
    {
        const uint64_t *g = sites + (s >> 6) * 3 * n_vars;
        for (int d = 0; d < 3; ++d)
            if (g[d * n_vars + v] >> (s & 63) & 1) return d;
        return -1;
    }
    int operator()(size_t n_vars, size_t G, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, int flush, mg_ibd_seg *segs, size_t cap, uint64_t *needed)
    {
        ++calls;
        most_vars = std::max(most_vars, n_vars);
        CHECK(G == (S + 63) / 64);
        std::vector<Pair> next = state;
        std::vector<mg_ibd_seg> out;
        size_t k = 0;
        for (size_t a = 0; a < S; ++a)
            for (size_t b = a + 1; b < S; ++b, ++k) {
                Pair &p = next[k];
                auto close = [&] {
                    if (p.open && p.n >= min_records && (long long)p.end - (long long)p.start >= min_bp)
                        out.push_back(mg_ibd_seg{(uint32_t)a, (uint32_t)b, p.chrom, p.start, p.end, p.n, p.ibs2, 0});
                    p.open = false;
                };
                for (size_t v = 0; v < n_vars; ++v) {
                    const int da = dosage(sites, n_vars, v, a), db = dosage(sites, n_vars, v, b);
                    if (p.open && p.chrom != chrom[v]) close();
                    if (da < 0 || db < 0) continue;
                    if (da + db == 2 && da != db) {
                        close();
                        continue;
                    }
                    if (!p.open) p = Pair{true, chrom[v], pos[v], pos[v], 0, 0};
                    p.end = pos[v], ++p.n, p.ibs2 += da == db;
                }
                if (flush) close();
            }
        *needed = out.size();
        if (out.size() > cap) {
            ++limits;
            return MG_ERR_LIMIT;
        }
        std::copy(out.begin(), out.end(), segs);
        state.swap(next);
        flushes += flush != 0;
        return MG_OK;
    }
};

struct Record {
    std::string cols;
    std::vector<int> dosage; // [samples], -1: no contribution
};

static void text_rules()
{
    std::string out;
    ibd_row(out, "s1", "s2", "chr1", mg_ibd_seg{0, 1, 0, 100, 1100, 7, 5, 0});
    ibd_row(out, "a", "b b", "2", mg_ibd_seg{3, 9, 4, 5, 5, 1, 0, 0});
    ibd_row(out, "a", "b", "X", mg_ibd_seg{0, 1, 0, 0, 4294967295u, 4294967295u, 4294967295u, 0});
    ibd_row(out, "a", "b", "X", mg_ibd_seg{0, 1, 0, 500, 100, 2, 2, 0});
    CHECK(out == "s1\ts2\tchr1\t100\t1100\t1000\t7\t5\n" "a\tb b\t2\t5\t5\t0\t1\t0\n" "a\tb\tX\t0\t4294967295\t4294967295\t4294967295\t4294967295\n" "a\tb\tX\t500\t100\t-400\t2\t2\n");
    CHECK(std::string(ibd_header()) == "#A\tB\tCHROM\tSTART\tEND\tLENGTH\tN\tIBS2\n");
}

// n records on three contigs (one name comes back: a contig id is a running number), positions 10 apart; sample s is the other homozygote where
// (v + 3 s) % 11 == 0, heterozygous or out now and then
static std::vector<Record> records(size_t n, size_t S)
{
    std::vector<Record> recs;
    uint32_t pos = 100;
    for (size_t v = 0; v < n; ++v) {
        Record r;
        const char *contig = v < n / 3 ? "chrA" : v < 2 * n / 3 ? "chrB" : "chrA";
        if (v == n / 3 || v == 2 * n / 3) pos = 50;
        pos += 10;
        r.cols = std::string(contig) + "\t" + std::to_string(pos) + "\t" + (v % 4 ? "id" + std::to_string(v) : ".") + "\tA\tC";
        for (size_t s = 0; s < S; ++s) {
            const uint64_t h = 0x9E3779B97F4A7C15ull * (v * 131 + s + 1) >> 40;
            r.dosage.push_back(h % 29 == 0 ? -1 : h % 13 == 0 ? 1 : (v + 3 * s) % 11 == 0 ? 2 : 0);
        }
        recs.push_back(r);
    }
    return recs;
}
// the groups' streams: group g holds the next sizes[g] samples in its low bits
static std::vector<std::string> streams(const std::vector<Record> &recs, const std::vector<size_t> &sizes)
{
    std::vector<std::string> out(sizes.size());
    for (const Record &r : recs) {
        size_t s0 = 0;
        for (size_t g = 0; g < sizes.size(); ++g) {
            uint64_t w[3] = {0, 0, 0};
            for (size_t p = 0; p < sizes[g]; ++p)
                if (r.dosage[s0 + p] >= 0) w[r.dosage[s0 + p]] |= 1ull << p;
            put_site_words(out[g], w[0], w[1], w[2], 2, g ? nullptr : r.cols.data(), r.cols.size());
            s0 += sizes[g];
        }
    }
    return out;
}
static std::vector<std::string> sample_names(size_t S)
{
    std::vector<std::string> names;
    for (size_t s = 0; s < S; ++s) names.push_back("sample" + std::to_string(s));
    return names;
}
// the whole table from the dosages themselves, pair by pair, without words, reader or sort
static std::string expected(const std::vector<Record> &recs, size_t S, uint32_t min_records, long long min_bp)
{
    const std::vector<std::string> names = sample_names(S);
    std::string out = ibd_header();
    for (size_t a = 0; a < S; ++a)
        for (size_t b = a + 1; b < S; ++b) {
            Pair p;
            std::string chrom_name;
            auto close = [&] {
                if (p.open && p.n >= min_records && (long long)p.end - (long long)p.start >= min_bp)
                    ibd_row(out, names[a], names[b], chrom_name, mg_ibd_seg{0, 0, 0, p.start, p.end, p.n, p.ibs2, 0});
                p.open = false;
            };
            for (const Record &r : recs) {
                const size_t t0 = r.cols.find('\t');
                const std::string contig = r.cols.substr(0, t0);
                const uint32_t pos = (uint32_t)atoi(r.cols.c_str() + t0 + 1);
                const int da = r.dosage[a], db = r.dosage[b];
                if (p.open && contig != chrom_name) close();
                if (da < 0 || db < 0) continue;
                if (da + db == 2 && da != db) {
                    close();
                    continue;
                }
                if (!p.open) p = Pair{true, 0, pos, pos, 0, 0}, chrom_name = contig;
                p.end = pos, ++p.n, p.ibs2 += da == db;
            }
            close();
        }
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
static std::string run_pass(const std::string &dir, const std::vector<std::string> &contents, const std::vector<size_t> &sizes, size_t S, size_t chunk, Fake &fake)
{
    const std::string path = dir + "/ibd.tsv";
    {
        std::deque<PartFile> files;
        PartFile table;
        fill(files, path, contents);
        table.open(path);
        ibd_table(files, sizes, sample_names(S), chunk, fake, [&](const char *data, size_t n) { table.write(data, n); });
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
        std::cerr << "usage: ibd_out_host_check SCRATCH_DIR\n";
        return 2;
    }
    const std::string dir = argv[1];
    text_rules();
    const size_t N = 90;
    {   // seventy samples, two words of cohort-wide bits, under four groupings
        const size_t S = 70;
        const std::vector<Record> recs = records(N, S);
        const std::vector<std::vector<size_t>> groupings = {{64, 6}, {35, 35}, {10, 20, 40}, std::vector<size_t>(70, 1)};
        const std::vector<std::pair<uint32_t, long long>> thresholds = {{3, 0}, {1, 0}, {4, 100}};
        size_t tables_seen = 0;
        for (const auto &[min_records, min_bp] : thresholds) {
            const std::string want = expected(recs, S, min_records, min_bp);
            const size_t lines = std::count(want.begin(), want.end(), '\n');
            CHECK(lines > (min_bp ? 100u : 2000u));
            tables_seen += tables_seen == 0 || want != expected(recs, S, thresholds[0].first, thresholds[0].second);
            for (const std::vector<size_t> &sizes : groupings) {
                const std::vector<std::string> contents = streams(recs, sizes);
                for (size_t chunk : {(size_t)1, (size_t)7, (size_t)30, (size_t)64, (size_t)89, (size_t)90, (size_t)91, (size_t)500}) {
                    if (sizes.size() == 70 && chunk != 7 && chunk != 500) continue; // (seventy streams: two chunk sizes will do)
                    Fake fake(S, min_records, min_bp);
                    CHECK(run_pass(dir, contents, sizes, S, chunk, fake) == want);
                    CHECK(fake.most_vars <= chunk && fake.flushes == 1);
                    CHECK(fake.calls - fake.limits == N / chunk + 1); // (a table that ends on a chunk's edge takes one more step, empty, to flush)
                    if (!min_bp && chunk == 500) CHECK(fake.limits == 1); // (the first buffer holds 1024 segments: the step came again, and the refused one moved nothing)
                }
            }
        }
        CHECK(tables_seen == 3); // (the thresholds change the table)
    }
    for (const std::vector<size_t> &sizes : std::vector<std::vector<size_t>>{std::vector<size_t>{5}, {2, 3}, {1, 4}, {1, 1, 1, 1, 1}}) { // a small cohort: no step outgrows the buffer
        const std::vector<Record> recs = records(N, 5);
        const std::string want = expected(recs, 5, 2, 0);
        CHECK(std::count(want.begin(), want.end(), '\n') > 20);
        for (size_t chunk : {(size_t)1, (size_t)45, (size_t)1000}) {
            Fake fake(5, 2, 0);
            CHECK(run_pass(dir, streams(recs, sizes), sizes, 5, chunk, fake) == want && fake.limits == 0);
        }
        Fake fake(5, 2, 0); // no record at all: one empty step that flushes, the header alone
        CHECK(run_pass(dir, std::vector<std::string>(sizes.size()), sizes, 5, 5, fake) == ibd_header() && fake.calls == 1 && fake.flushes == 1 && fake.most_vars == 0);
    }
    {   // one sample: no pair, no step, the header alone
        const std::vector<Record> recs = records(N, 1);
        Fake fake(2, 1, 0);
        CHECK(run_pass(dir, streams(recs, {1}), {1}, 1, 10, fake) == ibd_header() && fake.calls == 0);
    }
    {   // streams cut short, longer than the first, or of another record: an error, the table never under its name, nothing left
        const std::vector<size_t> sizes = {2, 3};
        const std::vector<Record> recs = records(N, 5);
        const std::vector<std::string> contents = streams(recs, sizes);
        const std::string path = dir + "/ibd.tsv";
        auto failing = [&](std::vector<std::string> bad, const char *why_piece) {
            const std::string why = error_of([&] {
                std::deque<PartFile> files;
                PartFile table;
                fill(files, path, bad);
                table.open(path);
                Fake fake(5, 2, 0);
                ibd_table(files, sizes, sample_names(5), 4, fake, [&](const char *data, size_t n) { table.write(data, n); });
                table.finish();
            });
            CHECK(has(why, why_piece));
            CHECK(!exists(path) && !exists(path + ".part") && !exists(path + ".g0.sites.part") && !exists(path + ".g1.sites.part"));
        };
        for (size_t g = 0; g < 2; ++g) {
            std::vector<std::string> bad = contents;
            bad[g].resize(bad[g].size() - 3);
            failing(bad, "IBD table are short");
        }
        std::vector<std::string> bad = contents;
        bad[1] += bad[1]; // more records than the first group has
        failing(bad, "IBD table are short");
        bad = contents;
        const uint32_t other = 5;
        memcpy(&bad[1][24], &other, 4); // a record with another number of alleles
        failing(bad, "IBD table are short");
        // a segment that names no pair: the pass refuses it
        const std::string why = error_of([&] {
            std::deque<PartFile> files;
            fill(files, path, contents);
            ibd_table(files, sizes, sample_names(5), 1000,
                      [](size_t, size_t, const uint64_t *, const uint32_t *, const uint32_t *, int, mg_ibd_seg *segs, size_t, uint64_t *needed) {
                          segs[0] = mg_ibd_seg{3, 3, 0, 1, 2, 1, 1, 0};
                          *needed = 1;
                          return MG_OK;
                      },
                      [](const char *, size_t) {});
        });
        CHECK(has(why, "names no pair"));
        CHECK(!exists(path + ".g0.sites.part"));
    }
    std::cout << "ibd_out_host_check: ok\n";
    return 0;
}
