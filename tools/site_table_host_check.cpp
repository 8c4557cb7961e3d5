// The host half of `call --cohort --site-stats` (malva_amd/host/cohort_out.hpp) driven without a device: the table's text on hand-written counts,
// the groups' count streams written and read back across 1, 2 and 3 groups with a made-up test in the device's place, streams cut short, and the
// PATH.part hand-over.  Meant to be built with -fsanitize=address,undefined and run on the CPU (`make sanitize-host`); tests/test_site_table_cpu.py
// builds it plain.  It takes a scratch directory as its argument and exits non-zero on the first wrong answer.
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
            std::cout << "site_table_host_check: FAILED\n";                    \
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

// in the device's place: values that show every input, exactly representable
static size_t fake_calls = 0, fake_items = 0;
static void fake_hwe(size_t n_items, const uint32_t *n, const uint32_t *het, const uint32_t *hom, double *hwe, double *exc)
{
    ++fake_calls;
    fake_items += n_items;
    for (size_t i = 0; i < n_items; ++i) hwe[i] = 1.0 / (1.0 + het[i]), exc[i] = (double)hom[i] / (double)(n[i] ? n[i] : 1);
}

struct Record {
    std::string cols;
    uint32_t A;
    std::vector<std::vector<uint32_t>> n_het_hom; // per group: n, het[A], hom[A]
};

static void text_rules()
{
    const char *cols = "c1\t7\t.\tA\tC,G";
    std::string out;
    const uint32_t het[3] = {3, 1, 2}, hom[3] = {0, 1, 0};
    const double p[2] = {0.5, 1e-7}, e[2] = {1.0, 0.123456789};
    site_stats_row(out, cols, strlen(cols), 70, false, 3, 3, het, hom, p, e);
    CHECK(out == "c1\t7\t.\tA\tC,G\t70\t3\t6\t3,2\t0.5,0.333333\t1,0\t1,2\t0.5,1e-07\t1,0.123457\n");
    out.clear();
    site_stats_row(out, cols, strlen(cols), 70, true, 3, 3, het, hom, nullptr, nullptr); // haploid: AC = hom, no test
    CHECK(out == "c1\t7\t.\tA\tC,G\t70\t3\t3\t1,0\t0.333333,0\t1,0\t1,2\t.,.\t.,.\n");
    out.clear();
    const uint32_t zero[2] = {0, 0};
    site_stats_row(out, "c\t1\t.\tA\tT", 9, 2, false, 2, 0, zero, zero, p, e); // nothing usable: AF and the tests are '.'
    CHECK(out == "c\t1\t.\tA\tT\t2\t0\t0\t0\t.\t0\t0\t.\t.\n");
    out.clear();
    site_stats_row(out, cols, strlen(cols), 70, false, 1, 3, het, hom, p, e); // no ALT: no line
    CHECK(out.empty());
    auto af = [](uint64_t ac, uint64_t an) {
        std::string s;
        site_stats_af(s, ac, an);
        return s;
    };
    CHECK(af(0, 0) == "." && af(0, 4) == "0" && af(4, 4) == "1" && af(1, 4) == "0.25" && af(2, 3) == "0.666667" && af(1, 3) == "0.333333");
    CHECK(af(1, 2000000) == "0.000001" && af(1, 2000001) == "0" && af(999999, 1000000) == "0.999999" && af(1999999, 2000000) == "1" && af(3999999, 4000000) == "1" && af(1, 16) == "0.0625");
    CHECK(site_stats_cols("c1\t7\t.\tA\tC,G\t.") == strlen(cols) && site_stats_cols("c1\t7") == 4 && site_stats_cols("") == 0);
    CHECK(std::string(site_stats_header()) == "#CHROM\tPOS\tID\tREF\tALT\tSAMPLES\tN\tAN\tAC\tAF\tHOM\tHET\tHWE\tEXC_HET\n");
}

static std::vector<Record> records(size_t groups)
{
    std::vector<Record> recs;
    const uint32_t As[] = {2, 1, 3, 2, 9, 2, 2};
    for (size_t v = 0; v < sizeof As / sizeof *As; ++v) {
        Record r;
        r.A = As[v];
        r.cols = "c" + std::to_string(v % 2) + "\t" + std::to_string(100 + v) + "\t.\tA\t";
        for (uint32_t a = 1; a < r.A; ++a) r.cols += (a > 1 ? "," : "") + std::string(a, 'T');
        if (r.A == 1) r.cols += ".";
        for (size_t g = 0; g < groups; ++g) {
            std::vector<uint32_t> c(1 + 2 * r.A);
            c[0] = v == 3 ? 0 : (uint32_t)(10 * (g + 1) + v); // (record 3: no usable cell in any group)
            for (uint32_t a = 0; a < r.A; ++a) c[1 + a] = c[0] ? (uint32_t)(a + g) : 0, c[1 + r.A + a] = c[0] ? (uint32_t)(v + a * g) % 5 : 0;
            r.n_het_hom.push_back(c);
        }
        recs.push_back(r);
    }
    return recs;
}
static std::vector<std::string> streams(const std::vector<Record> &recs, size_t groups)
{
    std::vector<std::string> out(groups);
    for (const Record &r : recs)
        for (size_t g = 0; g < groups; ++g) {
            const auto &c = r.n_het_hom[g];
            put_site_geno(out[g], r.A, c[0], &c[1], &c[1 + r.A], g ? nullptr : r.cols.data(), r.cols.size());
        }
    return out;
}
static std::string expected(const std::vector<Record> &recs, size_t groups, size_t samples, bool haploid)
{
    std::string out = site_stats_header();
    for (const Record &r : recs) {
        std::vector<uint32_t> sum(1 + 2 * r.A, 0), in, ih, io;
        for (size_t g = 0; g < groups; ++g)
            for (size_t i = 0; i < sum.size(); ++i) sum[i] += r.n_het_hom[g][i];
        site_stats_items(r.A, sum[0], &sum[1], &sum[1 + r.A], in, ih, io);
        std::vector<double> p(in.size()), e(in.size());
        const size_t calls = fake_calls, items = fake_items;
        fake_hwe(in.size(), in.data(), ih.data(), io.data(), p.data(), e.data());
        fake_calls = calls, fake_items = items;
        site_stats_row(out, r.cols.data(), r.cols.size(), samples, haploid, r.A, sum[0], &sum[1], &sum[1 + r.A], p.data(), e.data());
    }
    return out;
}
static void fill(std::deque<PartFile> &files, const std::string &base, const std::vector<std::string> &contents)
{
    for (size_t g = 0; g < contents.size(); ++g) {
        files.emplace_back();
        files.back().open(base + ".g" + std::to_string(g) + ".geno.part", PartFile::SCRATCH);
        files.back().write(contents[g]);
        files.back().finish();
    }
}
// the pass as the driver runs it: the table through a PartFile, the groups' streams gone before it takes its name
static std::string run_pass(const std::string &dir, const std::vector<std::string> &contents, size_t samples, bool haploid, size_t batch)
{
    const std::string path = dir + "/t.tsv";
    {
        std::deque<PartFile> files;
        PartFile table;
        fill(files, path, contents);
        table.open(path);
        site_stats_groups(files, samples, haploid, batch, fake_hwe, [&](const char *data, size_t n) { table.write(data, n); });
        CHECK(!exists(path) && exists(path + ".part"));
        files.clear();
        table.finish();
    }
    CHECK(exists(path) && !exists(path + ".part"));
    for (size_t g = 0; g < contents.size(); ++g) CHECK(!exists(path + ".g" + std::to_string(g) + ".geno.part"));
    const std::string text = slurp(path);
    unlink(path.c_str());
    return text;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::cerr << "usage: site_table_host_check SCRATCH_DIR\n";
        return 2;
    }
    const std::string dir = argv[1];
    text_rules();
    for (size_t groups = 1; groups <= 3; ++groups) {
        const std::vector<Record> recs = records(groups);
        const std::vector<std::string> contents = streams(recs, groups);
        const std::string want = expected(recs, groups, 10 * groups, false);
        CHECK(has(want, "\n") && std::count(want.begin(), want.end(), '\n') == 7); // the header and six records with an ALT
        for (size_t batch : {(size_t)1, (size_t)2, (size_t)7, (size_t)100}) {
            fake_calls = fake_items = 0;
            CHECK(run_pass(dir, contents, 10 * groups, false, batch) == want);
            CHECK(fake_items == 14); // 1 + 0 + 2 + 1 + 8 + 1 + 1 ALTs, every one tested once
            CHECK(fake_calls == (batch == 1 ? 6 : batch == 2 ? 4 : 1)); // (a batch without items makes no call)
        }
        fake_calls = 0;
        CHECK(run_pass(dir, contents, 10 * groups, true, 3) == expected(recs, groups, 10 * groups, true));
        CHECK(fake_calls == 0); // haploid: no test

        // streams cut short, or longer than the first: an error, the table never under its name, nothing left
        const std::string path = dir + "/t.tsv";
        auto failing = [&](std::vector<std::string> bad) {
            const std::string why = error_of([&] {
                std::deque<PartFile> files;
                PartFile table;
                fill(files, path, bad);
                table.open(path);
                site_stats_groups(files, 4, false, 2, fake_hwe, [&](const char *data, size_t n) { table.write(data, n); });
                table.finish();
            });
            CHECK(has(why.c_str(), "per-record table are short"));
            CHECK(!exists(path) && !exists(path + ".part") && !exists(path + ".g0.geno.part"));
        };
        for (size_t g = 0; g < groups; ++g) {
            std::vector<std::string> bad = contents;
            bad[g].resize(bad[g].size() - 3);
            failing(bad);
            if (!g) continue; // (the first stream cut at a record's end is a shorter panel, not an error of its own)
            bad = contents;
            bad[g].resize(bad[g].size() / 2);
            failing(bad);
        }
        if (groups > 1) {
            std::vector<std::string> bad = contents;
            bad[groups - 1] += bad[groups - 1]; // more records than the first group has
            failing(bad);
            bad = contents;
            uint32_t other = 5;
            memcpy(&bad[1][0], &other, 4); // a record with another number of alleles
            failing(bad);
        }
    }
    std::cout << "site_table_host_check: ok\n";
    return 0;
}
