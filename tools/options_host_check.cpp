// The command line of malva-geno (malva_amd/host/options.hpp, usage.hpp) driven without the program around it: a list of command
// lines, each run through parse_arguments into a string stream and rendered as one record -- the argv, whether it was accepted, the
// messages ahead of the usage and, when accepted, every field of Options that differs from its default, by name (the defaults, every
// field of them, are the file's first line).  The records are compared with
// tests/golden/options_cases.jsonl, which was recorded from the parser as it stood inside main.cpp before it became a table: a
// record that differs is a fault of the parser, not of the file.
//   options_host_check [GOLDEN]   compare (the default GOLDEN: tests/golden/options_cases.jsonl), then the checks of -h
//   options_host_check --dump     print the records
//   options_host_check --usage    print the usage text
// Meant to be built with -fsanitize=address,undefined and run on the CPU (`make sanitize-host`).
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "options.hpp"
#include "usage.hpp"

#define HOST_CHECK_NAME "options_host_check"
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond "\n";       \
            std::cout << HOST_CHECK_NAME ": FAILED\n";                         \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

using namespace malva;
using Args = std::vector<std::string>;

struct Case {
    Args argv;           // behind the sub-command
    const char *bf_bits; // MALVA_GENO_BF_BITS, or nullptr
};
static std::vector<Case> cases;

static void add_bare(const Args &args, const char *bf_bits = nullptr)
{
    for (const Case &c : cases)
        if (c.argv == args && !c.bf_bits && !bf_bits) return; // (the generated lists overlap here and there)
    cases.push_back({args, bf_bits});
}
// the options, then the three positional arguments
static void add(Args args, const char *bf_bits = nullptr)
{
    for (const char *p : {"a", "b", "c"}) args.push_back(p);
    add_bare(args, bf_bits);
}
static Args operator+(Args a, const Args &b)
{
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

// a bounded number: its ends, one beyond them, and the texts a reader may trip over (20 and 21 characters last)
static void add_number(const Args &with, const std::string &opt, const std::string &below, const std::string &lo, const std::string &hi, const std::string &above,
                       const Args &more = {})
{
    for (const std::string &text : Args{lo, hi, below, above, "", "+1", "-1", lo + "x", "00000000000000000001", "000000000000000000001"} + more) add(with + Args{opt, text});
}

static void make_cases()
{
    const Args C{"--cohort", "-o", "o"}, M{"--cohort", "--merged", "m"};
    add({});
    // ---- every option once, in every spelling, with what it goes with ----
    for (const Args &a : {Args{"-k", "31"}, {"--kmer-size", "31"}, {"-k31"}, {"--kmer-size=31"}, {"-r", "41"}, {"--ref-kmer-size", "41"}, {"-e", "0.01"}, {"--error-rate", "0.01"},
                          {"-s", "names.txt"}, {"--samples", "names.txt"}, {"-f", "EUR_AF"}, {"--freq-key", "EUR_AF"}, {"-c", "100"}, {"--max-coverage", "100"}, {"-b", "2"},
                          {"--bf-size", "2"}, {"-p"}, {"--strip-chr", "x"}, {"-u"}, {"--uniform", "x"}, {"-v"}, {"--verbose"}, {"-1"}, {"--haploid"}, {"--haplod"}, {"--hap"},
                          {"-d", "3"}, {"--device", "3"}, {"-g", "2"}, {"--gpus", "2"}, {"-puv1"}, {"-vk", "31"}, {"--min-count", "3"}, {"--max-count", "100"},
                          {"--min-count", "0", "--max-count", "4294967295"}})
        add(a);
    add({"--cohort", "-o", "out"});
    add({"--cohort", "--out-dir", "out"});
    add({"--cohort", "-o", ""}); // (-o has no emptiness check of its own)
    add({"--cohort", "-o", "", "--merged", "m.vcf"});
    add(C + Args{"--cohort-group", "8"});
    add(M);
    add({"--cohort", "--merged", "-"});
    add(M + Args{"-o", "out"});
    for (const Args &a : {Args{"--min-gq", "20"}, {"--site-tags"}, {"--merged-format", "bcf"}, {"--merged-f", "bcf"}, {"--gp"}, {"--pl"}, {"--pl", "--pl-cap", "99"},
                          {"--gp", "--pl", "--site-tags", "--min-gq", "5", "-v", "-1"}})
        add(M + a);
    for (const char *table : {"--pairs", "--sample-stats", "--site-stats", "--ld", "--ibd", "--grm"}) {
        add(C + Args{table, "t.tsv"});
        add(M + Args{table, "t.tsv"});
        add(C + Args{table, ""});
        add({table, ""});
    }
    for (const Args &a : {Args{"--ld-window", "10"}, {"--ld-window-bp", "5000"}, {"--ld-min-r2", "0.5"}, {"--ld-min-n", "4"},
                          {"--ld-window", "10", "--ld-window-bp", "5000", "--ld-min-r2", "0.5", "--ld-min-n", "4"}})
        add(C + Args{"--ld", "l.tsv"} + a);
    for (const Args &a : {Args{"--ibd-min-records", "10"}, {"--ibd-min-bp", "5000"}, {"--ibd-min-records", "10", "--ibd-min-bp", "5000"}}) add(C + Args{"--ibd", "i.tsv"} + a);
    for (const Args &a : {Args{"--grm-min-maf", "0.05"}, {"--grm-min-n", "4"}, {"--grm-format", "gcta"}, {"--grm-min-maf", "0.05", "--grm-min-n", "4", "--grm-format", "tsv"}})
        add(C + Args{"--grm", "g"} + a);
    for (const Args &a : {Args{}, {"--prior-iters", "3"}, {"--prior-weight", "2.5"}, {"--priors-out", "p.tsv"}, {"--prior-groups"},
                          {"--prior-iters", "0", "--prior-weight", "0", "--priors-out", "p.tsv", "--prior-groups"}})
        add(C + Args{"--cohort-priors"} + a);
    add(M + Args{"--cohort-priors", "--gp", "--pl", "--pairs", "a.tsv", "--sample-stats", "b.tsv", "--site-stats", "c.tsv", "--ld", "d.tsv", "--ibd", "e.tsv", "--grm", "f.tsv"});
    add({"-b", "1"}, "1024"); // MALVA_GENO_BF_BITS, read after a successful parse
    add({}, "0");
    add({}, "x");
    add({"--gpus", "0"}, "1024");
    // ---- what the reference leaves unchecked, and stays so ----
    for (const Args &a : {Args{"-k", "31z"}, {"-k", "z"}, {"-k", ""}, {"-k", "-1"}, {"-r", "41.5"}, {"-e", "1e-2x"}, {"-e", "x"}, {"-s", "two words"}, {"-s", ""}, {"-f", " AF"},
                          {"-c", "0"}, {"-b", "0"}, {"-b", "x"}, {"-b", "4x"}, {"-d", "-1"}, {"-d", "x"}, {"-g", "2x"}, {"-g", "x"}, {"-g", ""}})
        add(a);
    for (const char *g : {"0", "1", "64", "65", "-1", "99999999999"}) add({"--gpus", g});
    // ---- the bounded numbers ----
    add_number(C + Args{"--ld", "l"}, "--ld-window", "0", "1", "1024", "1025");
    add_number(C + Args{"--ld", "l"}, "--ld-window-bp", "-1", "0", "18446744073709551615", "18446744073709551616", {"10000000000000000000", "99999999999999999999"});
    add_number(C + Args{"--ld", "l"}, "--ld-min-n", "0", "1", "4294967295", "4294967296");
    add_number(C + Args{"--ibd", "i"}, "--ibd-min-records", "0", "1", "4294967295", "4294967296");
    add_number(C + Args{"--ibd", "i"}, "--ibd-min-bp", "-1", "0", "9223372036854775807", "9223372036854775808", {"18446744073709551615", "18446744073709551616"});
    add_number(C + Args{"--grm", "g"}, "--grm-min-n", "0", "1", "4294967295", "4294967296", {"00000000001", "0000000001"});
    add_number(C, "--cohort-group", "0", "1", "64", "65");
    for (const char *t : {"0", "1", "65", "x", "99999999999"}) add({"--cohort-group", t}); // (a refused value may still raise the "go with" line)
    add_number({}, "--min-count", "-1", "0", "4294967295", "4294967296");
    add_number({}, "--max-count", "-1", "0", "4294967295", "4294967296");
    add_number(M + Args{"--pl"}, "--pl-cap", "0", "1", "2147483647", "2147483648");
    add_number(M, "--min-gq", "-2147483649", "-2147483648", "2147483647", "2147483648");
    add_number(C + Args{"--cohort-priors"}, "--prior-iters", "-1", "0", "64", "65");
    for (const char *t : {"3x", "x3", "2y"}) {
        add({"--min-count", t});
        add({"--max-count", t});
        add(C + Args{"--cohort-group", t});
    }
    for (const char *t : {"0", "0.", ".5", "0.5", "0.500000", "0.500001", "0.5000000", "1", ".", "", "0,1", "1e-2", "00.1", "-0", "0.1 ", "0.000001"})
        add(C + Args{"--grm", "g", "--grm-min-maf", t});
    for (const char *t : {"0", "1", "1.0000001", "-0", "nan", "0.2x", "", "1e-1", "-0.1", " 0.5", "0.5 "}) add(C + Args{"--ld", "l", "--ld-min-r2", t});
    for (const char *t : {"-2147483648", "2147483647", "-2147483649", "2147483648", "-2147483647", "2147483646", "12x", "12 ", "", " 12", "12.0"})
        add(M + Args{"--min-gq", t});
    for (const char *t : {"1", "255", "2147483647", "0", "-1", "2147483648", "x", "", "1.5", "99 ", "9x", "99999999999999999999"}) { // (tests/test_pl_cpu.py)
        add(M + Args{"--pl", "--pl-cap", t});
    }
    for (const char *t : {"vcf", "bcf", "ubcf", "BCF", "bam", ""}) {
        add(M + Args{"--merged-format", t});
        add({"--merged-format", t});
    }
    for (const char *t : {"tsv", "gcta", "GCTA", "plink", ""}) {
        add(C + Args{"--grm", "g", "--grm-format", t});
        add({"--grm-format", t});
    }
    for (const char *t : {"007", "5x", " ", "1e1"}) add(C + Args{"--cohort-priors", "--prior-iters", t});
    for (const char *t : {"2.5", "0", "-0", "1e-3", "", "-1", "nan", "inf", "1e999", "1w"}) add(C + Args{"--cohort-priors", "--prior-weight", t});
    add(C + Args{"--cohort-priors", "--priors-out", ""});
    add({"--priors-out", ""});
    // ---- every "goes with" and "needs": alone, and with what it asks for ----
    add({"--cohort"});
    add({"--cohort", "--merged", ""});
    add({"--merged", ""});
    add({"--merged", "m.vcf"});
    add({"--merged", "-"});
    add({"-o", "out"});
    add({"--out-dir", "out"});
    add({"--cohort-group", "8"});
    add({"-o", "out", "--cohort-group", "8"});
    add({"--cohort", "--cohort-group", "8"});
    for (const Args &a : {Args{"--min-gq", "20"}, {"--site-tags"}, {"--min-gq", "20", "--site-tags"}, {"--merged-format", "bcf"}, {"--gp"}, {"--pl"}, {"--pl-cap", "99"},
                          {"--pl", "--pl-cap", "99"}}) {
        add(a);
        add(C + a);
        add(Args{"--cohort", "--merged", ""} + a);
    }
    add(M + Args{"--pl-cap", "99"});
    add(C + Args{"--gpus", "2"});
    add(M + Args{"-g", "64"});
    add({"--cohort", "--gpus", "2"});
    add({"--cohort", "--gpus", "65"});
    for (const char *table : {"--pairs", "--sample-stats", "--site-stats", "--ld", "--ibd", "--grm"}) add({table, "t.tsv"});
    for (const Args &a : {Args{"--ld-window", "10"}, {"--ld-window-bp", "5000"}, {"--ld-min-r2", "0.5"}, {"--ld-min-n", "4"}, {"--ld-window", "10", "--ld-min-n", "4"},
                          {"--ibd-min-records", "10"}, {"--ibd-min-bp", "5000"}, {"--ibd-min-records", "10", "--ibd-min-bp", "5000"}, {"--grm-min-maf", "0.05"},
                          {"--grm-min-n", "4"}, {"--grm-format", "gcta"}, {"--grm-format", "tsv"}, {"--grm-min-maf", "0.05", "--grm-format", "gcta"}}) {
        add(a);
        add(C + a);
        add(Args{"--ld", "l", "--ibd", "i", "--grm", "g"} + a);
    }
    add(C + Args{"--ld", "l", "--ibd-min-bp", "1"});
    add(C + Args{"--ibd", "i", "--grm-min-n", "1"});
    add(C + Args{"--grm", "g", "--ld-window", "1"});
    for (const Args &a : {Args{"--cohort-priors"}, {"--prior-iters", "3"}, {"--prior-weight", "2"}, {"--priors-out", "p.tsv"}, {"--prior-groups"},
                          {"--prior-iters", "3", "--prior-groups"}, {"--cohort-priors", "--prior-iters", "3"}}) {
        add(a);
        add(C + a);
    }
    // ---- a bad value and a missing parent; lines with three faults and more ----
    for (const Args &a : {Args{"--ld-window", "0"}, {"--ld-window-bp", "x"}, {"--ld-min-r2", "2"}, {"--ld-min-n", "0"}, {"--ibd-min-records", "0"}, {"--ibd-min-bp", "-1"},
                          {"--grm-min-maf", "0.6"}, {"--grm-min-n", "0"}, {"--grm-format", "x"}, {"--pl-cap", "0"}, {"--min-gq", "x"}, {"--merged-format", "x"},
                          {"--cohort-group", "65"}, {"--cohort-group", "x"}, {"--prior-iters", "65"}, {"--prior-weight", "-1"}, {"--priors-out", ""}}) {
        add(a);
        add(C + a);
    }
    add({"--ld-window", "0", "--gp"});
    add({"--ld-window", "0", "--gp", "--pl-cap", "0", "--grm-format", "x", "--ibd-min-bp", "1", "--gpus", "0", "--cohort-group", "70"});
    add({"--gpus", "65", "--cohort", "--min-gq", "1", "--merged-format", "bam", "--pl-cap", "3", "--pairs", "", "--prior-groups"});
    add_bare({"--grm-min-n", "00000000001", "--merged", "m", "--site-tags", "--ld", "l", "--ibd", "i", "--grm", "g", "-o", "out", "--cohort-priors", "--bogus", "a", "b"});
    add_bare({"--cohort", "--gpus", "2", "--merged", "", "--gp", "--pl", "--pl-cap", "x", "--ld-min-r2", "nan", "--sample-stats", "s", "a", "b", "c", "d"});
    add({"--min-count", "x", "--max-count", "-1", "--cohort-group", "0", "--min-gq", "", "-k", "31"});
    // ---- an option twice: the last path holds, an integer once taken stays taken ----
    for (const Args &a : {Args{"--merged", "m", "--merged", "", "--gp"}, {"--merged", "", "--merged", "m", "--gp"}, {"--pl-cap", "5", "--pl-cap", "0"}, {"--pl-cap", "0", "--pl-cap", "5"},
                          {"--min-gq", "5", "--min-gq", "x"}, {"--min-gq", "x", "--min-gq", "5"}, {"--ld", "l", "--ld", "", "--ld-window", "3"}, {"--merged-format", "bcf", "--merged-format", ""},
                          {"--merged-format", "x", "--merged-format", "vcf"}, {"--cohort-group", "65", "--cohort-group", "x"}, {"-k", "31", "-k", "33"}, {"-v", "-v"}}) {
        add(a);
        add(C + a);
    }
    // ---- positional arguments, unknown options, a missing argument ----
    add_bare({});
    add_bare({"a"});
    add_bare({"a", "b"});
    add_bare({"a", "b", "c"});
    add_bare({"a", "b", "c", "d"});
    add_bare({"a", "-v", "b", "--cohort", "c", "-o", "out"}); // (options between them)
    add_bare({"-v", "--", "a", "b", "-c"});
    add_bare({"--cohort", "a", "b"});
    add({"--bogus"});
    add({"-z"});
    add({"-vz"});
    add({"--min-"}); // (two long names begin so)
    add({"--verbose=1"});
    add_bare({"a", "b", "c", "--ld"});
    add_bare({"a", "b", "c", "-k"});
    add_bare({"a", "b", "c", "--strip-chr"});
    add_bare({"a", "b", "c", "--cohort", "--merged"});
}

static std::string quoted(const std::string &s)
{
    std::string out = "\"";
    char buf[8];
    for (const unsigned char ch : s) {
        if (ch == '"' || ch == '\\') out += '\\', out += (char)ch;
        else if (ch < 0x20 || ch >= 0x7f) snprintf(buf, sizeof buf, "\\u%04x", ch), out += buf;
        else out += (char)ch;
    }
    return out + "\"";
}
static std::string number(double v)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// every field of Options by name
static std::vector<std::pair<const char *, std::string>> fields(const Options &o)
{
    const auto n = [](auto v) { return std::to_string(v); };
    return {{"k", n(o.k)}, {"ref_k", n(o.ref_k)}, {"error_rate", number(o.error_rate)}, {"samples", quoted(o.samples)}, {"freq_key", quoted(o.freq_key)},
            {"max_coverage", n(o.max_coverage)}, {"bf_size", n(o.bf_size)}, {"strip_chr", n(o.strip_chr)}, {"uniform", n(o.uniform)}, {"verbose", n(o.verbose)},
            {"haploid", n(o.haploid)}, {"device", n(o.device)}, {"gpus", n(o.gpus)}, {"min_count", n(o.min_count)}, {"max_count", n(o.max_count)},
            {"fasta_path", quoted(o.fasta_path)}, {"vcf_path", quoted(o.vcf_path)}, {"kmc_path", quoted(o.kmc_path)}, {"cohort", n(o.cohort)}, {"out_dir", quoted(o.out_dir)},
            {"cohort_group", n(o.cohort_group)}, {"merged", quoted(o.merged)}, {"use_min_gq", n(o.use_min_gq)}, {"min_gq", n(o.min_gq)}, {"site_tags", n(o.site_tags)},
            {"merged_format", quoted(o.merged_format)}, {"gp", n(o.gp)}, {"pl", n(o.pl)}, {"pl_cap", n(o.pl_cap)}, {"pairs", quoted(o.pairs)},
            {"sample_stats", quoted(o.sample_stats)}, {"site_stats", quoted(o.site_stats)}, {"ld", quoted(o.ld)}, {"ld_window", n(o.ld_window)},
            {"ld_window_bp", n(o.ld_window_bp)}, {"ld_min_r2", number(o.ld_min_r2)}, {"ld_min_n", n(o.ld_min_n)}, {"ibd", quoted(o.ibd)},
            {"ibd_min_records", n(o.ibd_min_records)}, {"ibd_min_bp", n(o.ibd_min_bp)}, {"grm", quoted(o.grm)}, {"grm_maf_ppm", n(o.grm_maf_ppm)},
            {"grm_min_n", n(o.grm_min_n)}, {"grm_gcta", n(o.grm_gcta)}, {"priors.on", n(o.priors.on)}, {"priors.sub_given", n(o.priors.sub_given)},
            {"priors.iters", n(o.priors.iters)}, {"priors.weight", number(o.priors.weight)}, {"priors.out", quoted(o.priors.out)}, {"priors.groups", n(o.priors.groups)}};
}
// The fields as one JSON object.  all: every one of them -- the file's first line, the defaults; else those that differ from the
// defaults, so a field that moves when it should not, or stays when it should move, shows all the same
static std::string rendered(const Options &o, bool all)
{
    const auto is = fields(o), defaults = fields(Options());
    std::string r = "{";
    for (size_t i = 0; i < is.size(); ++i)
        if (all || is[i].second != defaults[i].second) r += (r.size() > 1 ? "," : "") + quoted(is[i].first) + ":" + is[i].second;
    return r + "}";
}

// one command line through the parser; `err` receives what it wrote
static Parsed run(const Case &c, Options &o, std::string &err)
{
    if (c.bf_bits) setenv("MALVA_GENO_BF_BITS", c.bf_bits, 1);
    else unsetenv("MALVA_GENO_BF_BITS");
    std::vector<std::string> words{"call"};
    words.insert(words.end(), c.argv.begin(), c.argv.end());
    std::vector<char *> argv;
    for (std::string &w : words) argv.push_back(&w[0]);
    argv.push_back(nullptr);
    // getopt starts afresh: it keeps a pointer into the last line it scanned, which is gone by now, and the parser's own optind = 1
    // does not drop it (a program parses one line and never meets this)
    optind = 0;
    getopt(1, argv.data(), "");
    std::ostringstream out;
    const Parsed p = parse_arguments((int)words.size(), argv.data(), o, out);
    err = out.str();
    return p;
}

static std::string record(const Case &c)
{
    Options o;
    std::string err;
    const Parsed p = run(c, o, err);
    CHECK(p == Parsed::ok || p == Parsed::bad);
    if (p == Parsed::bad) { // the messages, a blank line, the usage
        const std::string tail = std::string("\n") + USAGE;
        CHECK(err.size() >= tail.size() && err.compare(err.size() - tail.size(), tail.size(), tail) == 0); // (an unknown option: getopt alone spoke)
        err.resize(err.size() - tail.size());
    }
    std::string r = "{\"argv\":[";
    for (size_t i = 0; i < c.argv.size(); ++i) r += (i ? "," : "") + quoted(c.argv[i]);
    r += "],";
    if (c.bf_bits) r += "\"MALVA_GENO_BF_BITS\":" + quoted(c.bf_bits) + ",";
    r += std::string("\"accepted\":") + (p == Parsed::ok ? "true" : "false");
    std::istringstream lines(err);
    std::string says;
    for (std::string line; std::getline(lines, line);) says += (says.empty() ? "" : ",") + quoted(line);
    if (!says.empty()) r += ",\"messages\":[" + says + "]";
    if (p == Parsed::ok) r += ",\"options\":" + rendered(o, false);
    return r + "}";
}

int main(int argc, char **argv)
{
    const std::string arg = argc > 1 ? argv[1] : "";
    if (arg == "--usage") {
        std::cout << USAGE;
        return 0;
    }
    opterr = 0; // (getopt's own words about an unknown option go to the process's stderr, past the parser's stream: not here)
    make_cases();
    if (arg == "--dump") {
        std::cout << "{\"defaults\":" << rendered(Options(), true) << "}\n";
        for (const Case &c : cases) std::cout << record(c) << "\n";
        return 0;
    }
    const std::string golden = arg.empty() ? "tests/golden/options_cases.jsonl" : arg;
    std::ifstream in(golden);
    CHECK(in.good());
    std::string defaults;
    CHECK(std::getline(in, defaults) && defaults == "{\"defaults\":" + rendered(Options(), true) + "}");
    size_t n = 0;
    for (std::string want; std::getline(in, want); ++n) {
        CHECK(n < cases.size());
        const std::string got = record(cases[n]);
        if (got != want) {
            std::cerr << "case " << n + 1 << ":";
            for (const std::string &a : cases[n].argv) std::cerr << " " << quoted(a);
            std::cerr << "\n  recorded: " << want << "\n  now:      " << got << "\n";
            CHECK(got == want);
        }
    }
    CHECK(n == cases.size());
    // -h: nothing but what stood ahead of it is said, and the caller is told to print the usage
    for (const char *help : {"-h", "--help"}) {
        Options o;
        std::string err;
        CHECK(run({{"--ld-window", "0", "--bogus", help, "--grm-min-n", "0", "a", "b", "c", "d"}, nullptr}, o, err) == Parsed::help);
        CHECK(err == "malva : --ld-window takes a whole number 1..1024\n");
        CHECK(run({{help}, nullptr}, o, err) == Parsed::help && err.empty());
        CHECK(run({{"-k", "31", "a", "b", "c", help}, nullptr}, o, err) == Parsed::help && err.empty() && o.k == 31);
    }
    std::cout << HOST_CHECK_NAME ": ok\n";
    return 0;
}
