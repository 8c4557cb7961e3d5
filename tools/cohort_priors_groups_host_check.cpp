// The host side of `call --cohort --cohort-priors --prior-groups` (malva_amd/host/cohort_priors.hpp) driven without a device: the
// groups' coverage files and the cohort's frequency file written and walked back, with group sizes that do not divide 64, record
// ranges cut at record boundaries around a record of hundreds of alleles, mismatched stream or count headers refused, and the scratch
// removed when the frame is left by an exception.  The estimate is a stand-in that folds every plane's coverages into the outputs, so
// a wrong row, a wrong range or a wrong order shows.  Meant to be built with -fsanitize=address,undefined and run on the CPU
// (`make sanitize-host`); it exits non-zero on the first wrong answer.
#include <cstdio>
#include <deque>
#include <iostream>
#include <vector>

#include "cohort_priors.hpp"

static int failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond "\n";       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

struct MadeBatch {
    uint64_t stream;
    std::vector<uint32_t> vao;
    std::vector<float> f0;
    std::vector<uint32_t> cov; // [P][slots], the whole cohort's
};

static uint32_t cell(size_t batch, size_t plane, size_t slot) { return (uint32_t)(batch * 1000003u + plane * 7919u + slot * 31u + 1); }

// what the stand-in estimate makes of record v: order-sensitive in the planes
static void stand_in(size_t n, size_t P, const uint32_t *cov, const float *f0, const uint32_t *vao, float *f_t, uint32_t *n_inf)
{
    const size_t slots = vao[n];
    for (size_t v = 0; v < n; ++v) {
        uint32_t acc = 0;
        for (size_t pl = 0; pl < P; ++pl)
            for (uint32_t a = vao[v]; a < vao[v + 1]; ++a) acc = acc * 1664525u + cov[pl * slots + a];
        n_inf[v] = acc;
        for (uint32_t a = vao[v]; a < vao[v + 1]; ++a) f_t[a] = f0[a] + (float)(acc % 1000u + a - vao[v]);
    }
}

static bool exists(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (f) fclose(f);
    return f != nullptr;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const std::string base = dir + "/cohort_priors_groups_host_check";
    // the options
    {
        PriorOptions p;
        p.groups = true;
        CHECK(check_prior_options(p, true) == "--prior-groups goes with --cohort-priors");
        p.on = true;
        CHECK(check_prior_options(p, true).empty() && check_prior_options(p, false).find("--cohort-priors goes with --cohort") == 0);
        CHECK(prior_groups_error(1).empty() && prior_groups_error(65).empty() && prior_groups_error(MG_PRIOR_WIDE_MAX_PLANES).empty());
        CHECK(prior_groups_error(MG_PRIOR_WIDE_MAX_PLANES + 1).find("at most 16384 samples") != std::string::npos);
    }
    // range cuts: at record boundaries, a record that exceeds the bound a range of its own, nothing empty
    {
        const std::vector<uint32_t> vao{0, 2, 4, 304, 306, 309, 311};
        const auto all = cut_record_ranges(vao.data(), 6, 3, (size_t)1 << 30);
        CHECK(all == (std::vector<size_t>{0, 6}));
        const auto cuts = cut_record_ranges(vao.data(), 6, 3, 3 * 4 * 5); // five slots a range
        CHECK(cuts == (std::vector<size_t>{0, 2, 3, 5, 6}));
        const auto one = cut_record_ranges(vao.data(), 6, 3, 1); // every record by itself
        CHECK(one == (std::vector<size_t>{0, 1, 2, 3, 4, 5, 6}));
        CHECK(cut_record_ranges(vao.data(), 0, 3, 64) == std::vector<size_t>{0});
        CHECK(cut_record_ranges(vao.data(), 1, 70, 70 * 4 * 2) == (std::vector<size_t>{0, 1}));
    }
    // three batches (streams 0, 1, 1), the second with a record of 300 alleles; 70 planes in groups of 33, 31 and 6
    const std::vector<uint32_t> groups{33, 31, 6};
    const size_t P = 70;
    std::vector<MadeBatch> made(3);
    const std::vector<std::vector<uint32_t>> offs{{0, 2, 4, 7}, {0, 2, 302, 304, 307, 309}, {0, 8}};
    for (size_t b = 0; b < made.size(); ++b) {
        made[b].stream = b ? 1 : 0;
        made[b].vao = offs[b];
        const size_t slots = offs[b].back();
        made[b].f0.resize(slots);
        for (size_t a = 0; a < slots; ++a) made[b].f0[a] = (float)(b * 10 + a) / 1024.f;
        made[b].cov.resize(P * slots);
        for (size_t pl = 0; pl < P; ++pl)
            for (size_t a = 0; a < slots; ++a) made[b].cov[pl * slots + a] = cell(b, pl, a);
    }
    auto write_groups = [&](std::deque<PartFile> &files, int spoil) { // spoil: 0 none, 1 a stream, 2 a count, 3 a batch short, 4 a batch more
        size_t first = 0;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            files.emplace_back();
            files.back().open(base + ".g" + std::to_string(gi) + ".cov.part", PartFile::SCRATCH);
            for (size_t b = 0; b < made.size(); ++b) {
                if (spoil == 3 && gi == 1 && b == 2) continue;
                const size_t slots = made[b].vao.back(), n = made[b].vao.size() - 1;
                std::vector<uint32_t> rows(made[b].cov.begin() + first * slots, made[b].cov.begin() + (first + groups[gi]) * slots);
                std::string bytes;
                std::vector<uint32_t> vao = made[b].vao;
                uint64_t stream = made[b].stream;
                if (spoil == 1 && gi == 2 && b == 1) stream = 0;
                put_cov_batch(bytes, stream, n, vao.data(), made[b].f0.data(), gi == 0, groups[gi], rows.data());
                if (spoil == 2 && gi == 1 && b == 0) ++bytes[8]; // (n_records' low byte)
                files.back().write(bytes);
                if (spoil == 4 && gi == 2 && b == 2) files.back().write(bytes);
            }
            files.back().close();
            first += groups[gi];
        }
    };
    auto paths_of = [](const std::deque<PartFile> &files) {
        std::vector<std::string> paths;
        for (const auto &f : files) paths.push_back(f.path);
        return paths;
    };
    for (const size_t bound : {(size_t)1 << 30, (size_t)70 * 4 * 4, (size_t)1}) {
        std::deque<PartFile> files;
        write_groups(files, 0);
        PartFile freq;
        freq.open(base + ".freq.part", PartFile::SCRATCH);
        size_t calls = 0, most = 0;
        walk_prior_groups(paths_of(files), groups, bound,
                          [&](size_t n, size_t planes, const uint32_t *cov, const float *f0, const uint32_t *vao, float *f_t, uint32_t *n_inf) {
                              CHECK(planes == P && n > 0 && vao[0] == 0);
                              ++calls;
                              most = std::max<size_t>(most, vao[n]);
                              stand_in(n, planes, cov, f0, vao, f_t, n_inf);
                          },
                          [&](const std::string &bytes) { freq.write(bytes); });
        freq.close();
        CHECK(bound != ((size_t)1 << 30) || calls == 3);
        CHECK(bound != (size_t)70 * 4 * 4 || (calls == 2 + 5 + 1 && most == 300)); // {2,2}{3}; {2}{300}{2}{3}{2}; {8}
        CHECK(bound != 1 || calls == 3 + 5 + 1);
        // every group's output pass reads its rows and the cohort's values back
        size_t first = 0;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            PriorGroupInput in;
            in.open(files[gi].path, freq.path, groups[gi]);
            std::vector<uint32_t> cov, n_inf, want_n;
            std::vector<float> f_t, want_f;
            for (size_t b = 0; b < made.size(); ++b) {
                const size_t slots = made[b].vao.back(), n = made[b].vao.size() - 1;
                in.next(made[b].stream, n, slots, cov, f_t, n_inf);
                want_f.assign(slots, 0.f);
                want_n.assign(n, 0);
                stand_in(n, P, made[b].cov.data(), made[b].f0.data(), made[b].vao.data(), want_f.data(), want_n.data());
                CHECK(f_t == want_f && n_inf == want_n);
                CHECK(cov == std::vector<uint32_t>(made[b].cov.begin() + first * slots, made[b].cov.begin() + (first + groups[gi]) * slots));
            }
            in.done();
            first += groups[gi];
        }
        // a pass whose batches do not fit the streams is refused
        {
            PriorGroupInput in;
            in.open(files[1].path, freq.path, groups[1]);
            std::vector<uint32_t> cov, n_inf;
            std::vector<float> f_t;
            bool threw = false;
            try {
                in.next(1, 3, 7, cov, f_t, n_inf); // (the first batch is stream 0)
            } catch (const std::runtime_error &) {
                threw = true;
            }
            CHECK(threw);
            PriorGroupInput early;
            early.open(files[0].path, freq.path, groups[0]);
            early.next(0, 3, 7, cov, f_t, n_inf);
            threw = false;
            try {
                early.done(); // (two batches are left)
            } catch (const std::runtime_error &) {
                threw = true;
            }
            CHECK(threw);
        }
    }
    CHECK(!exists(base + ".g0.cov.part") && !exists(base + ".g2.cov.part") && !exists(base + ".freq.part"));
    // mismatched headers, a short and a long group: refused, and the scratch goes with the frame the exception leaves
    for (int spoil = 1; spoil <= 4; ++spoil) {
        bool threw = false;
        size_t sunk = 0;
        try {
            std::deque<PartFile> files;
            write_groups(files, spoil);
            PartFile freq;
            freq.open(base + ".freq.part", PartFile::SCRATCH);
            CHECK(exists(base + ".g1.cov.part") && exists(base + ".freq.part"));
            walk_prior_groups(paths_of(files), groups, (size_t)1 << 30, stand_in, [&](const std::string &bytes) {
                ++sunk;
                freq.write(bytes);
            });
        } catch (const std::runtime_error &e) {
            threw = std::string(e.what()).find("internal: ") == 0;
        }
        CHECK(threw);
        CHECK(sunk == (spoil == 1 ? 1u : spoil == 2 ? 0u : spoil == 3 ? 2u : 3u));
        for (size_t gi = 0; gi < groups.size(); ++gi) CHECK(!exists(base + ".g" + std::to_string(gi) + ".cov.part"));
        CHECK(!exists(base + ".freq.part"));
    }
    // the override of the bound
    setenv("MALVA_GENO_PRIOR_RANGE_BYTES", "4096", 1);
    CHECK(prior_range_bytes() == 4096);
    for (const char *bad : {"", "0", "x", "12x", "-"}) {
        setenv("MALVA_GENO_PRIOR_RANGE_BYTES", bad, 1);
        CHECK(prior_range_bytes() == PRIOR_RANGE_BYTES);
    }
    unsetenv("MALVA_GENO_PRIOR_RANGE_BYTES");
    CHECK(prior_range_bytes() == ((size_t)1 << 30));
    std::cout << (failures ? "cohort_priors_groups_host_check: FAILED\n" : "cohort_priors_groups_host_check: ok\n");
    return failures ? 1 : 0;
}
