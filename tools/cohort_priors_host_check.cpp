// The host side of `call --cohort --cohort-priors` (malva_amd/host/cohort_priors.hpp) driven without a device: the options' values
// and their checks, the one-group errors, the lines of --priors-out from a made-up batch, the PATH.part -> PATH hand-over.  Meant to
// be built with -fsanitize=address,undefined and run on the CPU (`make sanitize-host`); it exits non-zero on the first wrong answer.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
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

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    // values
    for (const char *good : {"0", "5", "64", "007"}) {
        PriorOptions p;
        CHECK(parse_prior_iters(good, p) && p.sub_given && p.iters == (uint32_t)atoi(good));
    }
    for (const char *bad : {"", "-1", "65", "5x", "x", " ", "1e1", "99999999999999999999999"}) {
        PriorOptions p;
        CHECK(!parse_prior_iters(bad, p) && p.sub_given && p.iters == 5);
    }
    {
        PriorOptions p;
        CHECK(!parse_prior_iters(nullptr, p) && !parse_prior_weight(nullptr, p) && !parse_priors_out(nullptr, p) && !parse_priors_out("", p));
        CHECK(parse_prior_weight("2.5", p) && p.weight == 2.5 && parse_prior_weight("0", p) && p.weight == 0 && parse_prior_weight("-0", p) && !std::signbit(p.weight));
        CHECK(parse_prior_weight("1e-3", p) && p.weight == 1e-3 && parse_priors_out("t.tsv", p) && p.out == "t.tsv");
    }
    for (const char *bad : {"", "-1", "nan", "inf", "-inf", "1e999", "w", "1w", "-1e-300"}) {
        PriorOptions p;
        CHECK(!parse_prior_weight(bad, p) && p.weight == 1.0);
    }
    // combinations
    {
        PriorOptions p;
        CHECK(check_prior_options(p, false).empty() && check_prior_options(p, true).empty());
        p.on = true;
        CHECK(check_prior_options(p, true).empty() && check_prior_options(p, false).find("--cohort-priors goes with --cohort") == 0);
        PriorOptions q;
        parse_prior_iters("3", q);
        CHECK(check_prior_options(q, true).find("--cohort-priors") != std::string::npos && check_prior_options(q, true).find("--prior-iters") != std::string::npos);
        q.on = true;
        CHECK(check_prior_options(q, true).empty());
    }
    CHECK(prior_group_error(3, 0).empty() && prior_group_error(64, 0).empty() && prior_group_error(3, 3).empty() && prior_group_error(3, 64).empty());
    CHECK(prior_group_error(65, 0).find("at most 64 samples") != std::string::npos && prior_group_error(65, 0).find("65") != std::string::npos);
    CHECK(prior_group_error(3, 2).find("--cohort-group 2") != std::string::npos && prior_group_error(3, 2).find("3 samples") != std::string::npos);
    CHECK(prior_memory_error(40).find("40 samples do not fit") != std::string::npos);
    // the table from a made-up batch: records of 2, 1, 3 and 9 alleles; a prefix with fewer columns than six; an empty one
    const std::vector<uint32_t> vao{0, 2, 3, 6, 15};
    std::vector<float> panel(15), cohort(15);
    for (size_t i = 0; i < panel.size(); ++i) {
        panel[i] = 0.003f * (float)(i + 1);
        cohort[i] = 1.0f / (float)(i + 3);
    }
    const std::vector<std::string> prefix{"1\t569\t.\tT\tC\t.", "1\t600\trs1\tG\t.\t30", "chr2\t7\t.\tCCA\tAAG,TGG\t.", "X\t1\t.\tA\tC,G,T,AA,AC,AG,AT,CA\t."};
    const uint32_t n_inf[4] = {4, 0, 64, 0};
    std::string text = priors_header();
    for (size_t v = 0; v < 4; ++v) priors_row(text, prefix[v], vao[v + 1] - vao[v], panel.data() + vao[v], cohort.data() + vao[v], n_inf[v]);
    priors_row(text, "short\t1", 2, panel.data(), cohort.data(), 1);
    priors_row(text, "", 0, nullptr, nullptr, 0);
    std::istringstream in(text);
    std::string line;
    std::vector<std::vector<std::string>> rows;
    while (std::getline(in, line)) {
        rows.emplace_back();
        std::istringstream cols(line);
        for (std::string c; std::getline(cols, c, '\t');) rows.back().push_back(c);
    }
    CHECK(rows.size() == 7 && rows[0].size() == 8 && rows[0][0] == "#CHROM" && rows[0][7] == "N_INFORMATIVE");
    for (size_t v = 0; v < 4 && rows.size() == 7; ++v) {
        const auto &r = rows[v + 1];
        CHECK(r.size() == 8 && r[7] == std::to_string(n_inf[v]));
        const uint32_t A = vao[v + 1] - vao[v];
        for (int col = 5; col < 7 && r.size() == 8; ++col) {
            if (A < 2) {
                CHECK(r[(size_t)col] == ".");
                continue;
            }
            std::istringstream list(r[(size_t)col]);
            uint32_t a = 1;
            for (std::string x; std::getline(list, x, ','); ++a) CHECK(a < A && (float)strtod(x.c_str(), nullptr) == (col == 5 ? panel : cohort)[vao[v] + a]); // the round trip
            CHECK(a == A);
        }
    }
    CHECK(rows.size() == 7 && rows[1][0] == "1" && rows[1][1] == "569" && rows[1][4] == "C" && rows[3][3] == "CCA" && rows[3][4] == "AAG,TGG");
    CHECK(rows.size() == 7 && rows[5][0] == "short" && rows[5][1] == "1");
    // the file: PATH.part while open, PATH at the end; PATH.part gone when the run ends early
    const std::string path = dir + "/cohort_priors_host_check.tsv";
    {
        PriorsFile f;
        f.write("ignored", 7); // (not open: nothing happens)
        f.open(path);
        CHECK(access((path + ".part").c_str(), F_OK) == 0 && access(path.c_str(), F_OK) != 0);
        f.write(text.data() + strlen(priors_header()), text.size() - strlen(priors_header()));
        f.finish();
        f.finish();
        CHECK(access((path + ".part").c_str(), F_OK) != 0);
    }
    {
        std::ifstream back(path);
        std::stringstream all;
        all << back.rdbuf();
        CHECK(all.str() == text);
    }
    unlink(path.c_str());
    {
        PriorsFile f;
        f.open(path);
    }
    CHECK(access((path + ".part").c_str(), F_OK) != 0 && access(path.c_str(), F_OK) != 0);
    {
        PriorsFile f;
        bool threw = false;
        try {
            f.open(dir + "/no/such/directory/t.tsv");
        } catch (const std::exception &) {
            threw = true;
        }
        CHECK(threw);
    }
    std::cout << (failures ? "cohort_priors_host_check: FAILED\n" : "cohort_priors_host_check: ok\n");
    return failures ? 1 : 0;
}
