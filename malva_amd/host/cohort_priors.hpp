// cohort_priors.hpp -- the host side of `call --cohort --cohort-priors`: the options' values and their checks, the reasons a
// cohort cannot run as one group, and the table of --priors-out; with --prior-groups the scratch streams of a cohort that runs as
// several groups (the groups' coverages, the cohort's frequencies) and the walk over them.  No device is needed for any of it: what
// needs one comes in as a callable (the sanitizer programs tools/cohort_priors_host_check.cpp and
// tools/cohort_priors_groups_host_check.cpp drive this file alone).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/malva_hip.h" // (MG_PRIOR_WIDE_MAX_PLANES; nothing here calls the library)
#include "part_file.hpp"

struct PriorOptions {
    bool on = false;      // --cohort-priors
    bool sub_given = false; // one of --prior-iters / --prior-weight / --priors-out was given
    uint32_t iters = 5;   // --prior-iters, 0..64
    double weight = 1.0;  // --prior-weight, finite and >= 0
    std::string out;      // --priors-out
    bool groups = false;  // --prior-groups: the cohort may run as several groups
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
    if (!p.on && p.groups) return "--prior-groups goes with --cohort-priors";
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

// ---- --prior-groups: a cohort in several groups ------------------------------------------------------------------------------------
// The estimate needs every sample's coverages of a record, the device holds one group's counters at a time.  So every group first
// leaves its coverages in a scratch file (BASE.gN.cov.part), a pass over all of these files makes the cohort's frequencies
// (BASE.freq.part), and a last pass per group reads both and makes the group's calls.  Every group sees the records in the same order
// and cuts them into the same batches; the streams are checked against each other all the same.
inline std::string prior_groups_error(size_t n_samples)
{
    if (n_samples > MG_PRIOR_WIDE_MAX_PLANES)
        return "--cohort-priors --prior-groups takes at most " + std::to_string((size_t)MG_PRIOR_WIDE_MAX_PLANES) + " samples: the manifest names " +
               std::to_string(n_samples);
    return std::string();
}

// one call's coverages stay under this many bytes: a batch is cut into record ranges (MALVA_GENO_PRIOR_RANGE_BYTES, when set: tests)
constexpr size_t PRIOR_RANGE_BYTES = (size_t)1 << 30;
inline size_t prior_range_bytes()
{
    const char *e = getenv("MALVA_GENO_PRIOR_RANGE_BYTES");
    if (!e || !*e) return PRIOR_RANGE_BYTES;
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return end == e || *end != '\0' || v == 0 ? PRIOR_RANGE_BYTES : (size_t)v;
}
// Records [0, n) cut into ranges at record boundaries so that planes rows of a range's slots take at most `bytes`; a record that
// exceeds them by itself is a range of its own.  -> the ranges' first records, then n
inline std::vector<size_t> cut_record_ranges(const uint32_t *var_allele_off, size_t n, size_t planes, size_t bytes)
{
    std::vector<size_t> cuts(1, 0);
    const size_t most = bytes / (4 * (planes ? planes : 1)); // slots a range may hold
    for (size_t v = 0; v < n; ++v)
        if ((size_t)(var_allele_off[v + 1] - var_allele_off[cuts.back()]) > most && v > cuts.back()) cuts.push_back(v);
    if (n) cuts.push_back(n);
    return cuts;
}

// A group's coverages, per batch and stream (the lone records', then the others'): the u64s stream, n_records, slots, has_panel; with
// has_panel (the first group) the u32s var_allele_off[n_records + 1] and the floats f0[slots]; then the u32s cov[planes][slots].
inline void put_cov_batch(std::string &out, uint64_t stream, uint64_t n_records, const uint32_t *var_allele_off, const float *f0, bool with_panel, size_t planes,
                          const uint32_t *cov)
{
    const uint64_t slots = var_allele_off[n_records], head[4] = {stream, n_records, slots, with_panel ? 1u : 0u};
    out.append((const char *)head, sizeof head);
    if (with_panel) {
        out.append((const char *)var_allele_off, 4 * (size_t)(n_records + 1));
        out.append((const char *)f0, 4 * (size_t)slots);
    }
    out.append((const char *)cov, 4 * planes * (size_t)slots);
}
// The cohort's frequencies, per batch and stream: the u64s stream, n_records, slots; the floats f_T[slots]; the u32s n_informative[n_records].
inline void put_freq_batch(std::string &out, uint64_t stream, uint64_t n_records, uint64_t slots, const float *f_t, const uint32_t *n_informative)
{
    const uint64_t head[3] = {stream, n_records, slots};
    out.append((const char *)head, sizeof head);
    out.append((const char *)f_t, 4 * (size_t)slots);
    out.append((const char *)n_informative, 4 * (size_t)n_records);
}

// a scratch stream open for reading
struct PriorStream {
    FILE *f = nullptr;
    PriorStream() = default;
    PriorStream(const PriorStream &) = delete;
    PriorStream &operator=(const PriorStream &) = delete;
    PriorStream(PriorStream &&o) noexcept : f(o.f) { o.f = nullptr; }
    ~PriorStream() { if (f) fclose(f); }
    void open(const std::string &path)
    {
        f = fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("cannot read " + path);
    }
    void read(void *to, size_t bytes, const char *what)
    {
        if (bytes && fread(to, 1, bytes, f) != bytes) throw std::runtime_error(what);
    }
    void seek(long long at, const char *what)
    {
        if (fseeko(f, (off_t)at, SEEK_SET) != 0) throw std::runtime_error(what);
    }
    bool at_end()
    {
        const int c = fgetc(f);
        if (c == EOF) return true;
        ungetc(c, f);
        return false;
    }
};

// The estimate pass: all groups' coverage files walked in step, batch by batch.  A batch's records are cut into ranges
// (cut_record_ranges over ALL planes of the cohort) and each range's coverages assembled as [P][range's slots] in the order of the
// groups -- the manifest's order; chunks of 64 planes are the estimate's affair, groups need not be multiples of 64 --
//   estimate(n_records, P, cov, f0, var_allele_off (from 0), f_t, n_informative)
// fills the range's part of the batch's f_T and n_informative, and sink(bytes) gets the batch as put_freq_batch makes it.  Memory: one
// range's coverages and a batch's records, whatever the cohort's size.
template <class Estimate, class Sink>
void walk_prior_groups(const std::vector<std::string> &paths, const std::vector<uint32_t> &group_planes, size_t range_bytes, Estimate &&estimate, Sink &&sink)
{
    const char *short_file = "internal: a group's coverages for the cohort's priors are short", *differ = "internal: the groups' coverages for the cohort's priors differ in their batches";
    if (paths.empty() || paths.size() != group_planes.size()) throw std::runtime_error(short_file);
    std::vector<PriorStream> in(paths.size());
    for (size_t gi = 0; gi < paths.size(); ++gi) in[gi].open(paths[gi]);
    size_t P = 0;
    for (uint32_t g : group_planes) P += g;
    std::vector<uint32_t> vao, range_vao, n_inf, cov;
    std::vector<float> f0, f_t;
    std::vector<long long> body(paths.size()); // where the batch's coverages start in every file
    std::string bytes;
    uint64_t head[4], h[4];
    while (!in[0].at_end()) {
        in[0].read(head, sizeof head, short_file);
        if (head[0] > 1 || head[3] != 1) throw std::runtime_error(differ);
        const size_t n = (size_t)head[1], slots = (size_t)head[2];
        vao.resize(n + 1);
        f0.resize(slots);
        in[0].read(vao.data(), 4 * (n + 1), short_file);
        in[0].read(f0.data(), 4 * slots, short_file);
        if (vao[0] != 0 || vao[n] != slots) throw std::runtime_error(differ);
        body[0] = ftello(in[0].f);
        for (size_t gi = 1; gi < in.size(); ++gi) {
            in[gi].read(h, sizeof h, short_file);
            if (h[0] != head[0] || h[1] != head[1] || h[2] != head[2] || h[3] != 0) throw std::runtime_error(differ);
            body[gi] = ftello(in[gi].f);
        }
        f_t.resize(slots);
        n_inf.resize(n);
        const std::vector<size_t> cuts = cut_record_ranges(vao.data(), n, P, range_bytes);
        for (size_t r = 0; r + 1 < cuts.size(); ++r) {
            const size_t r0 = cuts[r], r1 = cuts[r + 1], a0 = vao[r0], width = vao[r1] - a0;
            cov.resize(P * width);
            size_t row = 0;
            for (size_t gi = 0; gi < in.size(); ++gi)
                for (size_t pl = 0; pl < group_planes[gi]; ++pl, ++row) {
                    if (width != slots) in[gi].seek(body[gi] + 4 * (long long)(pl * slots + a0), short_file); // (a whole batch is read straight through)
                    in[gi].read(cov.data() + row * width, 4 * width, short_file);
                }
            range_vao.resize(r1 - r0 + 1);
            for (size_t v = r0; v <= r1; ++v) range_vao[v - r0] = vao[v] - (uint32_t)a0;
            estimate(r1 - r0, P, cov.data(), f0.data() + a0, range_vao.data(), f_t.data() + a0, n_inf.data() + r0);
        }
        for (size_t gi = 0; gi < in.size(); ++gi) in[gi].seek(body[gi] + 4 * (long long)(group_planes[gi] * slots), short_file);
        bytes.clear();
        put_freq_batch(bytes, head[0], n, slots, f_t.data(), n_inf.data());
        sink(bytes);
    }
    for (size_t gi = 1; gi < in.size(); ++gi)
        if (!in[gi].at_end()) throw std::runtime_error(differ);
}

// The output pass of one group: its coverage file and the cohort's frequency file read in step, in the order the pass cuts its batches.
struct PriorGroupInput {
    PriorStream cov, freq;
    size_t planes = 0;
    const char *short_file = "internal: the scratch of the cohort's priors is short", *differ = "internal: the scratch of the cohort's priors does not fit the panel's batches";
    void open(const std::string &cov_path, const std::string &freq_path, size_t group_planes)
    {
        cov.open(cov_path);
        freq.open(freq_path);
        planes = group_planes;
    }
    // the next batch of `stream` with n_records and slots: its coverages [planes][slots], the cohort's f_T[slots] and n_informative[n_records]
    void next(uint64_t stream, size_t n_records, size_t slots, std::vector<uint32_t> &cov_out, std::vector<float> &f_t, std::vector<uint32_t> &n_informative)
    {
        uint64_t h[4], q[3];
        cov.read(h, sizeof h, short_file);
        freq.read(q, sizeof q, short_file);
        if (h[0] != stream || h[1] != n_records || h[2] != slots || h[3] > 1 || q[0] != stream || q[1] != n_records || q[2] != slots) throw std::runtime_error(differ);
        if (h[3]) cov.seek(ftello(cov.f) + 4 * (long long)(n_records + 1 + slots), short_file); // (the panel's part: the pass has its own)
        cov_out.resize(planes * slots);
        f_t.resize(slots);
        n_informative.resize(n_records);
        cov.read(cov_out.data(), 4 * planes * slots, short_file);
        freq.read(f_t.data(), 4 * slots, short_file);
        freq.read(n_informative.data(), 4 * n_records, short_file);
    }
    // behind the last batch both streams are at their ends
    void done()
    {
        if (!cov.at_end() || !freq.at_end()) throw std::runtime_error(differ);
    }
};
