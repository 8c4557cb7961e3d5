// cohort_priors.hpp -- the host side of `call --cohort --cohort-priors`: the options' values and their checks, the reasons a
// cohort cannot run as one group, and the table of --priors-out.  No device is needed for any of it (the sanitizer program
// tools/cohort_priors_host_check.cpp drives this file alone).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "part_file.hpp"

struct PriorOptions {
    bool on = false;      // --cohort-priors
    bool sub_given = false; // one of --prior-iters / --prior-weight / --priors-out was given
    uint32_t iters = 5;   // --prior-iters, 0..64
    double weight = 1.0;  // --prior-weight, finite and >= 0
    std::string out;      // --priors-out
};

// --prior-iters N: a whole number 0..64 and nothing behind it
inline bool parse_prior_iters(const char *text, PriorOptions &p)
{
    p.sub_given = true;
    if (!text || !*text) return false;
    char *end = nullptr;
    const long long v = strtoll(text, &end, 10);
    if (end == text || *end != '\0' || v < 0 || v > 64) return false;
    p.iters = (uint32_t)v;
    return true;
}
// --prior-weight W: a finite number >= 0 and nothing behind it
inline bool parse_prior_weight(const char *text, PriorOptions &p)
{
    p.sub_given = true;
    if (!text || !*text) return false;
    char *end = nullptr;
    const double v = strtod(text, &end);
    if (end == text || *end != '\0' || !std::isfinite(v) || v < 0) return false;
    p.weight = v == 0 ? 0.0 : v; // (-0 is 0)
    return true;
}
inline bool parse_priors_out(const char *text, PriorOptions &p)
{
    p.sub_given = true;
    p.out = text ? text : "";
    return !p.out.empty();
}
// what is wrong with the combination, or the empty string
inline std::string check_prior_options(const PriorOptions &p, bool cohort)
{
    if (p.on && !cohort) return "--cohort-priors goes with --cohort";
    if (!p.on && p.sub_given) return "--prior-iters, --prior-weight and --priors-out go with --cohort-priors";
    return std::string();
}
// The estimate needs every sample of the cohort in one batch, so the cohort runs as ONE group: why the sizes alone forbid that, or the
// empty string (cohort_group: --cohort-group, 0 when not given)
inline std::string prior_group_error(size_t n_samples, int cohort_group)
{
    if (n_samples > 64)
        return "--cohort-priors needs the whole cohort in one group, and a group holds at most 64 samples: the manifest names " + std::to_string(n_samples);
    if (cohort_group && (size_t)cohort_group < n_samples)
        return "--cohort-priors needs the whole cohort in one group: --cohort-group " + std::to_string(cohort_group) + " is below the cohort's " +
               std::to_string(n_samples) + " samples";
    return std::string();
}
inline std::string prior_memory_error(size_t n_samples)
{
    return "--cohort-priors needs the whole cohort in one group: the counters of " + std::to_string(n_samples) +
           " samples do not fit on the device beside the index (a smaller cohort, or a run without --cohort-priors, fits)";
}

// One line of the table: CHROM POS ID REF ALT from the record's fixed columns (`prefix`: CHROM .. QUAL, tab-separated), then the ALT
// alleles' panel and cohort frequencies as comma lists (%.9g: a float survives the round trip; '.' for a record without ALT
// alleles) and the planes that counted.  panel / cohort: the record's n_alleles slots, REF first.
inline void priors_row(std::string &out, const std::string &prefix, uint32_t n_alleles, const float *panel, const float *cohort, uint32_t n_informative)
{
    size_t end = 0;
    for (int tabs = 0; end < prefix.size(); ++end)
        if (prefix[end] == '\t' && ++tabs == 5) break;
    out.append(prefix, 0, end);
    char num[48];
    for (const float *f : {panel, cohort}) {
        out += '\t';
        if (n_alleles < 2) out += '.';
        for (uint32_t a = 1; a < n_alleles; ++a) {
            snprintf(num, sizeof num, "%s%.9g", a > 1 ? "," : "", (double)f[a]);
            out += num;
        }
    }
    out += '\t';
    out += std::to_string(n_informative);
    out += '\n';
}
inline const char *priors_header() { return "#CHROM\tPOS\tID\tREF\tALT\tPANEL_AF\tCOHORT_AF\tN_INFORMATIVE\n"; }

// the table's file: a PartFile (PATH.part, renamed when the run is complete) that starts with the header line
struct PriorsFile : PartFile {
    void open(const std::string &p)
    {
        PartFile::open(p);
        write(priors_header(), strlen(priors_header()));
    }
};
