// The host half of `call --cohort --grm` (malva_amd/host/cohort_out.hpp) driven without a device: the rounding of the table's text on hand-written
// values, the groups' word streams written and read back under four groupings of one cohort of seventy samples -- 64 + 6, 35 + 35, 10 + 20 + 40 and
// seventy of one sample, whose words have to land in the same cohort-wide bits -- with the definition's loop (tools/grm_host_loop.cpp) in the
// device's place, chunk sizes from one record to the whole table, the text and GCTA's three files, streams cut short, and the PATH.part hand-over.
// Every grouping and chunk size must give the same bytes.  Meant to be built with -fsanitize=address,undefined and run on the CPU
// (`make sanitize-host`); tests/test_grm_out_cpu.py builds it plain.  It takes a scratch directory as its argument and exits non-zero on the first
// wrong answer.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>

#include "cohort_out.hpp"
#include "grm_host_loop.cpp"

using namespace malva;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond "\n";       \
            std::cout << "grm_out_host_check: FAILED\n";                       \
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

// In the device's place: mg_grm_begin's state, mg_grm_step and mg_grm_read
struct Fake {
    size_t S;
    int haploid;
    uint32_t maf_ppm, min_n;
    std::vector<int64_t> sum;
    std::vector<uint64_t> count;
    uint64_t seen = 0, entered = 0;
    size_t calls = 0, reads = 0, most_vars = 0;
    Fake(size_t S, int haploid, uint32_t maf_ppm, uint32_t min_n) : S(S), haploid(haploid), maf_ppm(maf_ppm), min_n(min_n), sum(S * (S + 1) / 2), count(S * (S + 1) / 2) {}
    void step(size_t n_vars, size_t G, const uint64_t *sites)
    {
        ++calls;
        most_vars = std::max(most_vars, n_vars);
        CHECK(G == (S + 63) / 64 && n_vars > 0);
        seen += n_vars;
        entered += grm_step_host(n_vars, (uint32_t)S, sites, haploid, maf_ppm, min_n, (uint32_t)S, sum.data(), count.data());
    }
    void read(int64_t *s, uint64_t *n, uint64_t *records)
    {
        ++reads;
        std::copy(sum.begin(), sum.end(), s);
        std::copy(count.begin(), count.end(), n);
        records[0] = seen, records[1] = entered;
    }
};

struct Record {
    std::string cols;
    std::vector<int> dosage; // [samples], -1: no contribution
};

static void text_rules()
{
    auto text = [](int64_t s, uint64_t n) {
        std::string out;
        grm_value(out, s, n);
        return out;
    };
    CHECK(text(0, 0) == "." && text(5, 0) == "." && text(0, 5) == "0.000000");
    CHECK(text(1 << 20, 1) == "1.000000" && text(-(1 << 20), 1) == "-1.000000");
    CHECK(text(1 << 19, 1 << 6) == "0.007813" && text(-(1 << 19), 1 << 6) == "-0.007813"); // 0.0078125, a tie: away from zero
    CHECK(text(-1, 4) == "0.000000" && text(1, 4) == "0.000000");                          // a value that rounds to zero has no sign
    CHECK(text(32608ll * 32608, 1) == "1014.024414");
    CHECK(text(INT64_MAX, 1) == "8796093022207.999999" && text(INT64_MIN, 1) == "-8796093022208.000000"); // (128 bits: nothing overflows)
    CHECK(text(INT64_MAX, UINT64_MAX >> 20) == "0.500000");
    CHECK(std::string(grm_header()) == "#A\tB\tN\tGRM\n");
}

// n records on two contigs; sample s carries the alternative allele by a hash, a record in nine is rare, one in seven has a cell out
static std::vector<Record> records(size_t n, size_t S, bool haploid)
{
    std::vector<Record> recs;
    for (size_t v = 0; v < n; ++v) {
        Record r;
        r.cols = std::string(v < n / 2 ? "chrA" : "chrB") + "\t" + std::to_string(100 + 10 * v) + "\t" + (v % 4 ? "id" + std::to_string(v) : ".") + "\tA\tC";
        for (size_t s = 0; s < S; ++s) {
            const uint64_t h = 0x9E3779B97F4A7C15ull * (v * 131 + s + 1) >> 40;
            const uint64_t cut = v % 9 == 0 ? 40 : 3 + v % 5;
            int d = h % 29 == 0 ? -1 : (h % cut == 0) + ((h >> 8) % cut == 0);
            if (haploid && d == 1) d = 2;
            if (v % 11 == 5) d = 0; // a monomorphic record
            r.dosage.push_back(d);
        }
        recs.push_back(r);
    }
    return recs;
}
// the groups' streams: group g holds the next sizes[g] samples in its low bits; the bits above them are set, which the pass must mask
static std::vector<std::string> streams(const std::vector<Record> &recs, const std::vector<size_t> &sizes)
{
    std::vector<std::string> out(sizes.size());
    for (const Record &r : recs) {
        size_t s0 = 0;
        for (size_t g = 0; g < sizes.size(); ++g) {
            uint64_t w[3] = {0, 0, 0};
            for (size_t p = 0; p < sizes[g]; ++p)
                if (r.dosage[s0 + p] >= 0) w[r.dosage[s0 + p]] |= 1ull << p;
            if (sizes[g] < 64)
                for (uint64_t &x : w) x |= ~0ull << sizes[g];
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
// the state from the dosages themselves, without words or reader
static GrmState expected(const std::vector<Record> &recs, size_t S, bool haploid, uint32_t maf_ppm, uint32_t min_n)
{
    GrmState st;
    st.sum.assign(S * (S + 1) / 2, 0), st.n.assign(S * (S + 1) / 2, 0);
    for (const Record &r : recs) {
        ++st.records[0];
        long long c[3] = {0, 0, 0};
        for (const int d : r.dosage)
            if (d >= 0) ++c[d];
        const long long n = c[0] + c[1] + c[2], an = haploid ? n : 2 * n, ac = haploid ? c[2] : c[1] + 2 * c[2], D = (haploid ? 4 : 2) * ac * (an - ac);
        if (D <= 0 || n < (long long)min_n || std::min(ac, an - ac) * 1000000 < (long long)maf_ppm * an) continue;
        long long q[3];
        bool fits = true;
        for (int d = 0; d < 3; ++d) q[d] = std::llrint((double)((d * an - 2 * ac) * 1024) / std::sqrt((double)D)), fits = fits && std::llabs(q[d]) <= MG_GRM_MAX_Q;
        if (!fits) continue;
        ++st.records[1];
        for (size_t a = 0, k = 0; a < S; ++a)
            for (size_t b = a; b < S; ++b, ++k)
                if (r.dosage[a] >= 0 && r.dosage[b] >= 0) st.sum[k] += q[r.dosage[a]] * q[r.dosage[b]], ++st.n[k];
    }
    return st;
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
static std::string run_pass(const std::string &dir, const std::vector<std::string> &contents, const std::vector<size_t> &sizes, size_t S, size_t chunk, Fake &fake, GrmState *state)
{
    const std::string path = dir + "/grm.tsv";
    {
        std::deque<PartFile> files;
        PartFile table;
        fill(files, path, contents);
        table.open(path);
        const GrmState st = grm_table(
            files, sizes, chunk, [&](size_t n_vars, size_t G, const uint64_t *sites) { fake.step(n_vars, G, sites); },
            [&](int64_t *s, uint64_t *n, uint64_t *records) { fake.read(s, n, records); });
        files.clear();
        for (size_t g = 0; g < contents.size(); ++g) CHECK(!exists(path + ".g" + std::to_string(g) + ".sites.part"));
        grm_text(st, sample_names(S), [&](const char *data, size_t n) { table.write(data, n); });
        CHECK(!exists(path) && exists(path + ".part"));
        table.finish();
        if (state) *state = st;
    }
    CHECK(exists(path) && !exists(path + ".part"));
    const std::string text = slurp(path);
    unlink(path.c_str());
    return text;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::cerr << "usage: grm_out_host_check SCRATCH_DIR\n";
        return 2;
    }
    const std::string dir = argv[1];
    text_rules();
    const size_t N = 90, S = 70;
    for (const bool haploid : {false, true}) { // seventy samples, two words of cohort-wide bits, under four groupings
        const std::vector<Record> recs = records(N, S, haploid);
        const std::vector<std::vector<size_t>> groupings = {{64, 6}, {35, 35}, {10, 20, 40}, std::vector<size_t>(70, 1)};
        std::string first;
        for (const auto &[maf_ppm, min_n] : std::vector<std::pair<uint32_t, uint32_t>>{{0, 1}, {100000, 66}}) {
            const GrmState want = expected(recs, S, haploid, maf_ppm, min_n);
            CHECK(want.records[0] == N && want.records[1] > 20 && want.records[1] <= N - 8); // (eight records are monomorphic)
            std::string want_text;
            grm_text(want, sample_names(S), [&](const char *data, size_t n) { want_text.append(data, n); });
            CHECK(std::count(want_text.begin(), want_text.end(), '\n') == 1 + S * (S + 1) / 2 && has(want_text, "\t-0.") && has(want_text, "sample3\tsample69\t"));
            if (first.empty()) first = want_text;
            else CHECK(first != want_text); // (the thresholds change the table)
            for (const std::vector<size_t> &sizes : groupings) {
                const std::vector<std::string> contents = streams(recs, sizes);
                for (size_t chunk : {(size_t)1, (size_t)7, (size_t)64, (size_t)89, (size_t)90, (size_t)91, (size_t)500}) {
                    if (sizes.size() == 70 && chunk != 7 && chunk != 500) continue; // (seventy streams: two chunk sizes will do)
                    Fake fake(S, haploid, maf_ppm, min_n);
                    GrmState got;
                    CHECK(run_pass(dir, contents, sizes, S, chunk, fake, &got) == want_text);
                    CHECK(got.sum == want.sum && got.n == want.n && got.records[0] == want.records[0] && got.records[1] == want.records[1]);
                    CHECK(fake.most_vars <= chunk && fake.reads == 1 && fake.calls == (N + chunk - 1) / chunk);
                }
            }
            // GCTA's files: the lower triangle row by row
            std::string bin, nbin, id;
            grm_gcta(
                want, sample_names(S), [&](const char *d, size_t n) { bin.append(d, n); }, [&](const char *d, size_t n) { nbin.append(d, n); },
                [&](const char *d, size_t n) { id.append(d, n); });
            CHECK(bin.size() == 4 * S * (S + 1) / 2 && nbin.size() == bin.size());
            size_t at = 0, zero_n = 0;
            for (size_t i = 0; i < S; ++i)
                for (size_t j = 0; j <= i; ++j, ++at) {
                    const size_t k = j * (2 * S - j + 1) / 2 + (i - j);
                    float v, c;
                    memcpy(&v, &bin[4 * at], 4), memcpy(&c, &nbin[4 * at], 4);
                    CHECK(c == (float)want.n[k]);
                    CHECK(v == (want.n[k] ? (float)((double)want.sum[k] / ((double)want.n[k] * 1048576.0)) : 0.f));
                    zero_n += !want.n[k];
                }
            CHECK(zero_n == 0 && has(id, "sample0\tsample0\nsample1\tsample1\n") && std::count(id.begin(), id.end(), '\n') == (long)S);
        }
    }
    {   // a pair that is never called together: N 0, `.`, 0 in GCTA's file; and no record at all: no step, one read, zeros
        std::vector<Record> recs = records(N, 3, false);
        for (size_t v = 0; v < N; ++v) recs[v].dosage[v % 2 ? 0 : 2] = -1;
        Fake fake(3, 0, 0, 1);
        const std::string text = run_pass(dir, streams(recs, {2, 1}), {2, 1}, 3, 16, fake, nullptr);
        CHECK(has(text, "sample0\tsample2\t0\t.\n") && !has(text, "sample0\tsample1\t0\t"));
        GrmState st = expected(recs, 3, false, 0, 1);
        std::string bin, nbin, id;
        grm_gcta(
            st, sample_names(3), [&](const char *d, size_t n) { bin.append(d, n); }, [&](const char *d, size_t n) { nbin.append(d, n); }, [&](const char *d, size_t n) { id.append(d, n); });
        float v = 1.f, c = 1.f;
        memcpy(&v, &bin[4 * 3], 4), memcpy(&c, &nbin[4 * 3], 4); // row 2, column 0
        CHECK(v == 0.f && c == 0.f && id == "sample0\tsample0\nsample1\tsample1\nsample2\tsample2\n");
        Fake none(3, 0, 0, 1);
        const std::string empty = run_pass(dir, std::vector<std::string>(2), {2, 1}, 3, 5, none, nullptr);
        CHECK(none.calls == 0 && none.reads == 1 && std::count(empty.begin(), empty.end(), '\n') == 7 && has(empty, "sample2\tsample2\t0\t.\n"));
    }
    {   // streams cut short, longer than the first, or of another record: an error, the table never under its name, nothing left
        const std::vector<size_t> sizes = {2, 3};
        const std::vector<Record> recs = records(N, 5, false);
        const std::vector<std::string> contents = streams(recs, sizes);
        const std::string path = dir + "/grm.tsv";
        auto failing = [&](std::vector<std::string> bad, const char *why_piece) {
            const std::string why = error_of([&] {
                std::deque<PartFile> files;
                PartFile table;
                fill(files, path, bad);
                table.open(path);
                Fake fake(5, 0, 0, 1);
                const GrmState st = grm_table(
                    files, sizes, 4, [&](size_t n_vars, size_t G, const uint64_t *sites) { fake.step(n_vars, G, sites); },
                    [&](int64_t *s, uint64_t *n, uint64_t *records) { fake.read(s, n, records); });
                grm_text(st, sample_names(5), [&](const char *data, size_t n) { table.write(data, n); });
                table.finish();
            });
            CHECK(has(why, why_piece));
            CHECK(!exists(path) && !exists(path + ".part") && !exists(path + ".g0.sites.part") && !exists(path + ".g1.sites.part"));
        };
        for (size_t g = 0; g < 2; ++g) {
            std::vector<std::string> bad = contents;
            bad[g].resize(bad[g].size() - 3);
            failing(bad, "GRM are short");
        }
        std::vector<std::string> bad = contents;
        bad[1] += bad[1]; // more records than the first group has
        failing(bad, "GRM are short");
        bad = contents;
        const uint32_t other = 5;
        memcpy(&bad[1][24], &other, 4); // a record with another number of alleles
        failing(bad, "GRM are short");
        const std::string why = error_of([&] { // names that are not the state's
            GrmState st;
            st.sum.resize(3), st.n.resize(3);
            try {
                grm_text(st, sample_names(3), [](const char *, size_t) {});
            } catch (const std::logic_error &e) {
                throw std::runtime_error(e.what());
            }
        });
        CHECK(has(why, "not the names'"));
    }
    std::cout << "grm_out_host_check: ok\n";
    return 0;
}
