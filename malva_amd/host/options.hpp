// What the command line of malva-geno says, once parsed, and the parser: one table with a row per option (OPTIONS), parse_arguments
#pragma once
#include <getopt.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <ostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/malva_hip.h" // (MG_LD_MAX_WINDOW; nothing here calls the library)
#include "cohort_priors.hpp"
#include "usage.hpp"

namespace malva {

struct Options { // argument_parser.hpp:51-66
    unsigned k = 35, ref_k = 43;
    float error_rate = 0.001f;
    std::string samples = "-", freq_key = "AF";
    unsigned max_coverage = 200;
    uint64_t bf_size = 1ULL << 35;
    bool strip_chr = false, uniform = false, verbose = false, haploid = false;
    int device = 0, gpus = 1;
    uint32_t min_count = 2, max_count = 255; // READS: KMC's -ci / -cs defaults (MALVA:107)
    std::string fasta_path, vcf_path, kmc_path;
    bool cohort = false;    // kmc_path is a manifest (host/cohort.hpp)
    std::string out_dir;    // -o
    int cohort_group = 0;   // 0: as many as fit, at most 64
    std::string merged;     // --merged: the multi-sample VCF ("-": stdout)
    bool use_min_gq = false; // --min-gq: cells of the merged output below it print a missing genotype
    int32_t min_gq = 0;
    bool site_tags = false; // --site-tags: AC / AN / AF / NS in the merged output's INFO
    std::string merged_format; // --merged-format: vcf (or empty: not given), bcf, ubcf
    bool gp = false;        // --gp: the genotype posteriors as the FORMAT field GP of the merged output
    bool pl = false;        // --pl: the prior-free Phred-scaled likelihoods as the FORMAT field PL of the merged output
    int32_t pl_cap = 255;   // --pl-cap: the largest PL written (the bcftools convention)
    std::string pairs;      // --pairs: the table of pairwise genotype sharing
    std::string sample_stats; // --sample-stats: the per-sample QC table
    std::string site_stats; // --site-stats: the per-record QC table
    std::string ld;         // --ld: the table of r2 between nearby records
    uint32_t ld_window = 64;        // --ld-window: the records behind a record that are its partners (1..MG_LD_MAX_WINDOW)
    uint64_t ld_window_bp = 1000000; // --ld-window-bp: and no further away than this (0: no limit)
    double ld_min_r2 = 0.2;         // --ld-min-r2: the smallest r2 written
    uint32_t ld_min_n = 2;          // --ld-min-n: the fewest samples a pair's r2 is formed from
    std::string ibd;        // --ibd: the table of IBS0-free segments per pair of samples
    uint32_t ibd_min_records = 100;   // --ibd-min-records: the fewest records of a segment written
    uint64_t ibd_min_bp = 1000000;    // --ibd-min-bp: and its smallest END - START (0: no limit)
    std::string grm;        // --grm: the genetic relationship matrix of the cohort's samples
    uint32_t grm_maf_ppm = 10000;     // --grm-min-maf: the smallest minor allele frequency of a record that enters, in parts per million
    uint32_t grm_min_n = 2;           // --grm-min-n: the fewest called samples of a record that enters
    bool grm_gcta = false;            // --grm-format gcta: PATH.grm.bin, PATH.grm.N.bin, PATH.grm.id instead of the text
    PriorOptions priors;    // --cohort-priors and its sub-options (host/cohort_priors.hpp)
};

// ---- one row per option ---------------------------------------------------------------------------------------------------------
enum OptArg { NO_ARG, ARG, LONG_ARG }; // LONG_ARG: the long name asks for an argument its letter does not take (the reference's quirk)
struct Opt {
    const char *name; // --name
    char letter;      // -l, or 0
    OptArg arg;
    // how the text is read and where the value goes; false: refused.  `given`: the option holds a value from the command line -- set
    // by the parser when the text is taken, left alone when it is refused (only a path takes it back, see there).  nullptr: -h
    bool (*read)(const char *text, Options &o, const Opt &row, bool &given);
    long long lo;          // a number's bounds ...
    unsigned long long hi;
    size_t width;          // ... and the longest text it is read from (digits)
    const char *says;      // "--name <says>" when the text is refused
    const char *parent;    // the option this one goes with: "--name goes with --parent"; the sub-options of --ld, --ibd and --grm
                           // share one message per parent, and count even when their text was refused
};

// the kinds of reading -------------------------------------------------------------------------------------------------------------
template <auto M> bool flag(const char *, Options &o, const Opt &, bool &)
{
    o.*M = true;
    return true;
}
// the reference's own: >> and no questions asked (-k 31z is 31, -k z is 0)
template <auto M> bool unchecked(const char *text, Options &o, const Opt &, bool &)
{
    std::istringstream(text) >> o.*M;
    return true;
}
inline bool read_bf_size(const char *text, Options &o, const Opt &row, bool &given)
{
    unchecked<&Options::bf_size>(text, o, row, given);
    o.bf_size *= 1ULL << 33; // "GB" on the command line, 2^33 bits each (argument_parser.hpp:119-123)
    return true;
}
template <auto M> bool any_text(const char *text, Options &o, const Opt &, bool &)
{
    o.*M = text;
    return true;
}
template <auto M> bool path(const char *text, Options &o, const Opt &, bool &given)
{
    o.*M = text;
    return given = *text != '\0'; // (an empty path is stored too, so it takes an earlier one away)
}
// a whole number lo..hi in at most `width` characters, digits only: strtoull would take a sign and wrap
template <auto M> bool digits(const char *text, Options &o, const Opt &row, bool &)
{
    const size_t n = strlen(text);
    unsigned long long v = 0;
    bool ok = n >= 1 && n <= row.width;
    for (const char *p = text; ok && *p; ++p) {
        ok = *p >= '0' && *p <= '9' && v <= (~0ull - (unsigned)(*p - '0')) / 10;
        if (ok) v = v * 10 + (unsigned)(*p - '0');
    }
    if (!ok || v < (unsigned long long)row.lo || v > row.hi) return false;
    o.*M = (std::remove_reference_t<decltype(o.*M)>)v;
    return true;
}
// an integer lo..hi read with >>; to_end: nothing but blanks may follow it (without: --min-count 3x is 3)
template <auto M, bool to_end> bool integer(const char *text, Options &o, const Opt &row, bool &)
{
    std::istringstream arg(text);
    long long v = 0;
    if (!(arg >> v) || (to_end && !(arg >> std::ws).eof()) || v < row.lo || v > (long long)row.hi) return false;
    o.*M = (std::remove_reference_t<decltype(o.*M)>)v;
    return true;
}
inline bool read_cohort_group(const char *text, Options &o, const Opt &, bool &)
{
    std::istringstream arg(text); // (read in place: a refused 65 stays, and "-o and --cohort-group go with --cohort" below sees it)
    return (arg >> o.cohort_group) && o.cohort_group >= 1 && o.cohort_group <= 64;
}
inline bool one_of(const char *text, std::initializer_list<const char *> words)
{
    for (const char *w : words)
        if (!strcmp(text, w)) return true;
    return false;
}
inline bool read_merged_format(const char *text, Options &o, const Opt &, bool &)
{
    o.merged_format = text;
    return one_of(text, {"vcf", "bcf", "ubcf"});
}
inline bool read_grm_format(const char *text, Options &o, const Opt &, bool &)
{
    if (!one_of(text, {"tsv", "gcta"})) return false;
    o.grm_gcta = !strcmp(text, "gcta");
    return true;
}
inline bool read_ld_min_r2(const char *text, Options &o, const Opt &, bool &)
{
    char *end = nullptr;
    const double v = strtod(text, &end);
    if (end == text || *end || !(v >= 0.0 && v <= 1.0)) return false;
    o.ld_min_r2 = v;
    return true;
}
// the decimal text read exactly: [D][.DDDDDD], parts per million
inline bool read_grm_min_maf(const char *text_, Options &o, const Opt &, bool &)
{
    const std::string text = text_;
    const size_t dot = text.find('.');
    const std::string head = text.substr(0, dot), tail = dot == std::string::npos ? std::string() : text.substr(dot + 1);
    bool ok = head.size() + tail.size() >= 1 && head.size() <= 1 && tail.size() <= 6;
    for (const char ch : head + tail) ok = ok && ch >= '0' && ch <= '9';
    if (!ok) return false;
    uint32_t ppm = head.empty() ? 0 : (uint32_t)(head[0] - '0') * 1000000u, scale = 100000;
    for (const char ch : tail) ppm += (uint32_t)(ch - '0') * scale, scale /= 10;
    if (ppm > 500000) return false;
    o.grm_maf_ppm = ppm;
    return true;
}
template <bool (*parse)(const char *, PriorOptions &)> bool prior(const char *text, Options &o, const Opt &, bool &) { return parse(text, o.priors); }

// The table.  Same short options and long names as the reference, including its quirks: --strip-chr / --uniform ask for an argument
// and --haploid is also spelt "haplod" (argument_parser.hpp:70-84).  A new option: a row here, a field of Options, a paragraph of the usage.
inline const Opt OPTIONS[] = {
    {"kmer-size", 'k', ARG, unchecked<&Options::k>},
    {"ref-kmer-size", 'r', ARG, unchecked<&Options::ref_k>},
    {"error-rate", 'e', ARG, unchecked<&Options::error_rate>},
    {"freq-key", 'f', ARG, unchecked<&Options::freq_key>},
    {"samples", 's', ARG, unchecked<&Options::samples>},
    {"max-coverage", 'c', ARG, unchecked<&Options::max_coverage>},
    {"bf-size", 'b', ARG, read_bf_size},
    {"strip-chr", 'p', LONG_ARG, flag<&Options::strip_chr>},
    {"uniform", 'u', LONG_ARG, flag<&Options::uniform>},
    {"verbose", 'v', NO_ARG, flag<&Options::verbose>},
    {"haplod", '1', NO_ARG, flag<&Options::haploid>},
    {"haploid", '1', NO_ARG, flag<&Options::haploid>},
    {"device", 'd', ARG, unchecked<&Options::device>},
    {"help", 'h', NO_ARG, nullptr},
    {"gpus", 'g', ARG, unchecked<&Options::gpus>},
    {"min-count", 0, ARG, integer<&Options::min_count, false>, 0, 0xFFFFFFFFull, 0, "takes a count 0..4294967295"},
    {"max-count", 0, ARG, integer<&Options::max_count, false>, 0, 0xFFFFFFFFull, 0, "takes a count 0..4294967295"},
    {"cohort", 0, NO_ARG, flag<&Options::cohort>},
    {"cohort-group", 0, ARG, read_cohort_group, 0, 0, 0, "takes 1..64"},
    {"out-dir", 'o', ARG, any_text<&Options::out_dir>},
    {"merged", 0, ARG, path<&Options::merged>, 0, 0, 0, "takes a path, or - for stdout", "cohort"},
    {"min-gq", 0, ARG, integer<&Options::min_gq, true>, INT32_MIN, INT32_MAX, 0, "takes an integer (int32)"},
    {"site-tags", 0, NO_ARG, flag<&Options::site_tags>},
    {"merged-format", 0, ARG, read_merged_format, 0, 0, 0, "takes vcf, bcf or ubcf"},
    {"gp", 0, NO_ARG, flag<&Options::gp>, 0, 0, 0, nullptr, "merged"},
    {"pairs", 0, ARG, path<&Options::pairs>, 0, 0, 0, "takes a path", "cohort"},
    {"sample-stats", 0, ARG, path<&Options::sample_stats>, 0, 0, 0, "takes a path", "cohort"},
    {"cohort-priors", 0, NO_ARG, [](const char *, Options &o, const Opt &, bool &) { return o.priors.on = true; }},
    {"prior-iters", 0, ARG, prior<parse_prior_iters>, 0, 0, 0, "takes a whole number 0..64"},
    {"prior-weight", 0, ARG, prior<parse_prior_weight>, 0, 0, 0, "takes a finite number >= 0"},
    {"priors-out", 0, ARG, prior<parse_priors_out>, 0, 0, 0, "takes a path"},
    {"prior-groups", 0, NO_ARG, [](const char *, Options &o, const Opt &, bool &) { return o.priors.groups = true; }},
    {"pl", 0, NO_ARG, flag<&Options::pl>, 0, 0, 0, nullptr, "merged"},
    {"pl-cap", 0, ARG, integer<&Options::pl_cap, true>, 1, INT32_MAX, 0, "takes a whole number 1..2147483647", "pl"},
    {"site-stats", 0, ARG, path<&Options::site_stats>, 0, 0, 0, "takes a path", "cohort"},
    {"ld", 0, ARG, path<&Options::ld>, 0, 0, 0, "takes a path", "cohort"},
    {"ld-window", 0, ARG, digits<&Options::ld_window>, 1, MG_LD_MAX_WINDOW, 20, "takes a whole number 1..1024", "ld"},
    {"ld-window-bp", 0, ARG, digits<&Options::ld_window_bp>, 0, ~0ull, 20, "takes a whole number (0: no limit)", "ld"},
    {"ld-min-r2", 0, ARG, read_ld_min_r2, 0, 0, 0, "takes a number in [0, 1]", "ld"},
    {"ld-min-n", 0, ARG, digits<&Options::ld_min_n>, 1, 0xFFFFFFFFull, 20, "takes a whole number 1..4294967295", "ld"},
    {"ibd", 0, ARG, path<&Options::ibd>, 0, 0, 0, "takes a path", "cohort"},
    {"ibd-min-records", 0, ARG, digits<&Options::ibd_min_records>, 1, 0xFFFFFFFFull, 20, "takes a whole number 1..4294967295", "ibd"},
    {"ibd-min-bp", 0, ARG, digits<&Options::ibd_min_bp>, 0, 0x7FFFFFFFFFFFFFFFull, 20, "takes a whole number (0: no limit)", "ibd"},
    {"grm", 0, ARG, path<&Options::grm>, 0, 0, 0, "takes a path", "cohort"},
    {"grm-min-maf", 0, ARG, read_grm_min_maf, 0, 0, 0, "takes a decimal number 0 .. 0.5 with at most six decimals", "grm"},
    {"grm-min-n", 0, ARG, digits<&Options::grm_min_n>, 1, 0xFFFFFFFFull, 10, "takes a whole number 1..4294967295", "grm"},
    {"grm-format", 0, ARG, read_grm_format, 0, 0, 0, "takes tsv or gcta", "grm"},
};
static_assert(MG_LD_MAX_WINDOW == 1024, "the message of --ld-window and the usage name the bound");
constexpr size_t N_OPTIONS = std::size(OPTIONS);

// what getopt answers for a row: its letter (both spellings of --haploid share theirs), without one 256 + its index
inline int option_code(size_t i) { return OPTIONS[i].letter ? OPTIONS[i].letter : 256 + (int)i; }
inline size_t option_row(const char *name)
{
    for (size_t i = 0; i < N_OPTIONS; ++i)
        if (!strcmp(OPTIONS[i].name, name)) return i;
    throw std::logic_error(std::string("no option --") + name);
}

// ok: `o` holds the command line.  bad: the messages and the usage went to `err`.  help: -h was met -- what stood ahead of it had
// its messages, the caller prints the usage to stdout and leaves with status 0
enum class Parsed { ok, bad, help };

inline Parsed parse_arguments(int argc, char **argv, Options &o, std::ostream &err)
{
    std::vector<option> longopts; // getopt's tables from ours
    std::string letters;
    for (size_t i = 0; i < N_OPTIONS; ++i) {
        const Opt &row = OPTIONS[i];
        longopts.push_back({row.name, row.arg == NO_ARG ? no_argument : required_argument, nullptr, option_code(i)});
        if (row.letter && letters.find(row.letter) == std::string::npos) letters += row.arg == ARG ? std::string{row.letter, ':'} : std::string{row.letter};
    }
    longopts.push_back({nullptr, 0, nullptr, 0});
    bool die = false;
    const auto say = [&](const std::string &what) {
        err << "malva : " << what << "\n";
        die = true;
    };
    bool seen[N_OPTIONS] = {}, given[N_OPTIONS] = {}; // met on the line, even when refused; holds a value from it
    optind = 1;
    for (int c; (c = getopt_long(argc, argv, letters.c_str(), longopts.data(), nullptr)) != -1;) {
        size_t i = 0;
        while (i < N_OPTIONS && option_code(i) != c) ++i;
        if (i == N_OPTIONS) { // '?': getopt has said why
            die = true;
            continue;
        }
        const Opt &row = OPTIONS[i];
        if (!row.read) return Parsed::help;
        seen[i] = true;
        if (row.read(optarg ? optarg : "", o, row, given[i])) given[i] = true;
        else say(std::string("--") + row.name + " " + row.says);
    }
    o.use_min_gq = given[option_row("min-gq")];

    // ---- what goes with what: the messages in the order they have always come ----
    const auto has = [&](const char *name) { return given[option_row(name)]; };
    const auto with_parent = [&](std::initializer_list<const char *> names) { // the regular ones, from the rows' parent column
        for (const char *name : names)
            if (const char *parent = OPTIONS[option_row(name)].parent; has(name) && !has(parent)) say(std::string("--") + name + " goes with --" + parent);
    };
    const auto sub_seen = [&](const char *parent) { // one of the rows whose parent it is was met, refused or not
        for (size_t i = 0; i < N_OPTIONS; ++i)
            if (seen[i] && OPTIONS[i].parent && !strcmp(OPTIONS[i].parent, parent)) return true;
        return false;
    };
    if (argc - optind < 3) say("missing arguments");
    else if (argc - optind > 3) say("too many arguments");
    if (o.gpus < 1 || o.gpus > 64) say("--gpus must be 1..64");
    if (o.cohort && o.out_dir.empty() && o.merged.empty()) say("--cohort needs -o OUTDIR or --merged PATH");
    with_parent({"merged"});
    if (!has("merged") && (has("min-gq") || has("site-tags"))) say("--min-gq and --site-tags go with --merged");
    if (!has("merged") && !o.merged_format.empty()) say("--merged-format goes with --merged"); // (a refused word counts, an empty one does not)
    with_parent({"gp", "pl", "pl-cap"});
    if (o.cohort && o.gpus > 1) say("--cohort does not combine with --gpus > 1");
    with_parent({"pairs", "sample-stats", "site-stats", "ld"});
    if (sub_seen("ld") && !has("ld")) say("--ld-window, --ld-window-bp, --ld-min-r2 and --ld-min-n go with --ld");
    with_parent({"ibd"});
    if (sub_seen("ibd") && !has("ibd")) say("--ibd-min-records and --ibd-min-bp go with --ibd");
    with_parent({"grm"});
    if (sub_seen("grm") && !has("grm")) say("--grm-min-maf, --grm-min-n and --grm-format go with --grm");
    if (const std::string why = check_prior_options(o.priors, o.cohort); !why.empty()) say(why);
    if (!o.cohort && (!o.out_dir.empty() || o.cohort_group)) say("-o and --cohort-group go with --cohort");
    if (die) {
        err << "\n" << USAGE;
        return Parsed::bad;
    }
    o.fasta_path = argv[optind++];
    o.vcf_path = argv[optind++];
    o.kmc_path = argv[optind++];
    if (const char *bits = getenv("MALVA_GENO_BF_BITS")) // tests: filters smaller than -b's 2^33-bit granule
        if (atoll(bits) > 0) o.bf_size = (uint64_t)atoll(bits);
    return Parsed::ok;
}

} // namespace malva
