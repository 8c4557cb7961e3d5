// What one batch of `call` does on the device (malva_amd/host/call_worker.hpp, malva_amd/host/device.hpp), driven on the CPU against an ABI
// of its own: this file defines struct mg_ctx and every mg_* entry point the worker calls, with the prototypes of include/malva_hip.h, and is
// linked WITHOUT libmalva_hip.  Every fake appends a line to its context's log -- its name, sizes, and its output pointers as offsets
// from the first one its batch passed -- and writes its WHOLE output range with a recognisable fill, so that a wrong size or offset is a
// sanitizer finding or a wrong line of text, not a silent pass.  Every expected value is written out here.  Built with
// -fsanitize=address,undefined and again with -fsanitize=thread by `make sanitize-host`; tests/test_call_worker_cpu.py builds it plain.
//     call_worker_host_check [SCRATCH-DIR]      (default: the current directory; what it writes there it removes)
#define HOST_CHECK_NAME "call_worker_host_check"
#include "host_check_util.hpp"

#include <condition_variable>
#include <cstdarg>
#include <fstream>
#include <sstream>

#include "call_worker.hpp"

using namespace malva;

// ---- the fake ABI ------------------------------------------------------------------------------------------------------------------------
struct Sync { // the pipeline case: an even batch waits for the odd batch behind it
    std::mutex mu;
    std::condition_variable cv;
    int odd_done = 0, active = 0, most_active = 0;
    bool timed_out = false;
};
struct mg_ctx {
    std::vector<std::string> log;
    std::string error = "fake: the device said no";
    uint32_t plane = 0;
    uint32_t n_planes = 1;              // what mg_cover_blocks_cohort fills
    const uint32_t *cov0 = nullptr;     // the batch's arrays, as its first call named them
    const int32_t *g10 = nullptr;
    const double *probs0 = nullptr;
    std::vector<size_t> flagged;        // the records the cover calls hand back
    uint64_t first_need = 0;            // not 0: the row formatters first answer MG_ERR_LIMIT with this need
    bool limit_said = false;
    int genotype_calls = 0, fail_genotype_at = 0; // mg_genotype number fail_genotype_at answers MG_ERR_HIP
    Sync *sync = nullptr;
    bool odd = false;
};
static void say(mg_ctx *c, const char *fmt, ...)
{
    char line[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    c->log.push_back(line);
}
template <class T> static void touch(const T *p, size_t n) // (reads the whole input range)
{
    volatile T sink = T();
    for (size_t i = 0; i < n; ++i) sink = p[i];
    (void)sink;
}

extern "C" {
int mg_destroy(mg_ctx *ctx)
{
    delete ctx;
    return MG_OK;
}
const char *mg_last_error(const mg_ctx *ctx) { return ctx->error.c_str(); }
int mg_cohort_select(mg_ctx *c, uint32_t plane)
{
    c->plane = plane;
    say(c, "mg_cohort_select %u", plane);
    return MG_OK;
}
int mg_call_isolated(mg_ctx *c, size_t n, const uint64_t *pos, const uint32_t *vao, const uint32_t *allele_off, const char *pool, size_t pool_len, const float *freq,
                     const uint64_t *present, const uint8_t *flags, float, int, int, uint32_t *cov_out, int32_t *gt1, int32_t *gt2, int32_t *gq, uint8_t *status, double *probs,
                     const uint64_t *var_gt_off)
{
    const size_t na = vao[n], ng = probs ? var_gt_off[n] : 0;
    touch(pos, n), touch(allele_off, na + 1), touch(pool, pool_len), touch(freq, na), touch(present, n), touch(flags, n);
    if (c->plane == 0) c->cov0 = cov_out, c->g10 = gt1, c->probs0 = probs;
    say(c, "mg_call_isolated n=%zu cov+%td g1+%td probs+%td", n, cov_out - c->cov0, gt1 - c->g10, probs ? probs - c->probs0 : (ptrdiff_t)-1);
    for (size_t i = 0; i < na; ++i) cov_out[i] = 10 * (c->plane + 1) + (uint32_t)i;
    for (size_t i = 0; i < n; ++i) gt1[i] = 0, gt2[i] = 1, gq[i] = 10 * ((int32_t)c->plane + 1) + (int32_t)i, status[i] = MG_GT_NORMAL;
    for (size_t i = 0; i < ng; ++i) probs[i] = 0.5;
    return MG_OK;
}
static int cover(mg_ctx *c, const char *name, const mg_blocks_host &x, uint32_t planes, uint32_t *cov_out, uint8_t *overflow)
{
    const size_t n = x.n_vars, na = x.var_allele_off[n]; // every member over its documented extent (mg_blocks_host)
    touch(x.blk_ref_base, x.n_blocks), touch(x.blk_ref_len, x.n_blocks), touch(x.blk_var_off, x.n_blocks + 1);
    touch(x.pos, n), touch(x.ref_size, n), touch(x.min_size, n), touch(x.present, n), touch(x.var_allele_off, n + 1);
    touch(x.allele_off, na + 1), touch(x.pool, x.pool_len), touch(x.canon, na);
    if (x.sp_off) touch(x.sp_off, n + 1), touch(x.sp_sample, x.sp_off[n]), touch(x.sp_gt, x.sp_off[n]);
    else touch(x.gt, n * x.n_samples);
    c->cov0 = cov_out, c->g10 = nullptr, c->probs0 = nullptr;
    say(c, "%s blocks=%zu n=%zu samples=%u dense=%d sparse=%d", name, x.n_blocks, n, x.n_samples, (int)(x.gt != nullptr), (int)(x.sp_off != nullptr));
    for (size_t pl = 0; pl < planes; ++pl)
        for (size_t i = 0; i < na; ++i) cov_out[pl * na + i] = 100 * ((uint32_t)pl + 1) + (uint32_t)i;
    for (size_t i = 0; i < n; ++i) overflow[i] = 0;
    for (size_t f : c->flagged) overflow[f] = 1;
    return MG_OK;
}
int mg_cover_blocks(mg_ctx *c, const mg_blocks_host *x, int, uint32_t *cov_out, uint8_t *overflow) { return cover(c, "mg_cover_blocks", *x, 1, cov_out, overflow); }
int mg_cover_blocks_cohort(mg_ctx *c, const mg_blocks_host *x, int, uint32_t *cov_out, uint8_t *overflow)
{
    return cover(c, "mg_cover_blocks_cohort", *x, c->n_planes, cov_out, overflow);
}
int mg_lookup_cover(mg_ctx *c, const char *rows, size_t stride, size_t n_rows, const uint8_t *is_ref, const uint64_t *sig_kmer_off, size_t n_sigs, const uint64_t *allele_sig_off,
                    size_t n_alleles, uint32_t *cov_out)
{
    touch(rows, n_rows * stride), touch(is_ref, n_rows), touch(sig_kmer_off, n_sigs + 1), touch(allele_sig_off, n_alleles + 1);
    if (!c->cov0) c->cov0 = cov_out; // (no cover call came first: every block goes this way, the first at slot 0)
    say(c, "mg_lookup_cover plane=%u cov+%td alleles=%zu", c->plane, cov_out - c->cov0, n_alleles);
    for (size_t a = 0; a < n_alleles; ++a) cov_out[a] = 70 + (uint32_t)a;
    return MG_OK;
}
int mg_genotype(mg_ctx *c, const uint32_t *cov, const float *freq, const uint32_t *vao, size_t n, float, int, int, int32_t *gt1, int32_t *gt2, int32_t *gq, uint8_t *status,
                double *probs, const uint64_t *var_gt_off)
{
    const size_t na = vao[n], ng = probs ? var_gt_off[n] : 0;
    touch(cov, na), touch(freq, na);
    ++c->genotype_calls;
    if (!c->cov0) c->cov0 = cov;
    if (cov == c->cov0) c->g10 = gt1, c->probs0 = probs;
    const int32_t pl = na ? (int32_t)((cov - c->cov0) / (ptrdiff_t)na) : 0;
    say(c, "mg_genotype n=%zu cov+%td g1+%td probs+%td id=%d", n, cov - c->cov0, gt1 - c->g10, probs ? probs - c->probs0 : (ptrdiff_t)-1, (int)freq[0]);
    if (c->genotype_calls == c->fail_genotype_at) return MG_ERR_HIP;
    if (c->sync) {
        Sync &s = *c->sync;
        std::unique_lock<std::mutex> lk(s.mu);
        s.most_active = std::max(s.most_active, ++s.active);
        if (c->odd) {
            s.odd_done = c->genotype_calls;
            s.cv.notify_all();
        } else if (!s.cv.wait_until(lk, std::chrono::system_clock::now() + std::chrono::seconds(30), // (the system clock: a wait ThreadSanitizer of GCC 11 knows)
                                    [&] { return s.odd_done >= std::min(c->genotype_calls, 2); })) // (the fifth batch has none behind it)
            s.timed_out = true;
        --s.active;
    }
    for (size_t i = 0; i < n; ++i) gt1[i] = 1, gt2[i] = 1, gq[i] = 50 + 10 * pl + (int32_t)i, status[i] = MG_GT_NORMAL;
    for (size_t i = 0; i < ng; ++i) probs[i] = 0.25;
    return MG_OK;
}
int mg_genotype_cohort(mg_ctx *c, size_t n, uint32_t planes, const uint32_t *cov, const float *freq, const uint32_t *vao, float, int, int, uint32_t iters, double weight,
                       float *freq_out, uint32_t *n_informative, int32_t *gt1, int32_t *gt2, int32_t *gq, uint8_t *status, double *probs, const uint64_t *var_gt_off)
{
    const size_t na = vao[n], ng = probs ? var_gt_off[n] : 0;
    touch(cov, planes * na);
    say(c, "mg_genotype_cohort n=%zu planes=%u iters=%u weight=%g freq_copy=%d probs=%d", n, planes, iters, weight,
        (int)(freq != freq_out && memcmp(freq, freq_out, 4 * na) == 0), (int)(probs != nullptr));
    for (size_t i = 0; i < na; ++i) freq_out[i] = iters ? 0.125f : freq[i];
    for (size_t i = 0; i < n; ++i) n_informative[i] = 99;
    for (size_t pl = 0; pl < planes; ++pl)
        for (size_t i = 0; i < n; ++i) gt1[pl * n + i] = 0, gt2[pl * n + i] = 0, gq[pl * n + i] = 70 + 10 * (int32_t)pl + (int32_t)i, status[pl * n + i] = MG_GT_NORMAL;
    for (size_t i = 0; i < planes * ng; ++i) probs[i] = 0.75;
    return MG_OK;
}
static int stats(mg_ctx *c, const char *name, float *ms_out, std::initializer_list<float> ms)
{
    say(c, "%s", name);
    for (float m : ms) *ms_out++ = m;
    return MG_OK;
}
int mg_format_stats(mg_ctx *c, float *ms) { return stats(c, "mg_format_stats", ms, {1, 2, 3}); }
int mg_bcf_stats(mg_ctx *c, float *ms) { return stats(c, "mg_bcf_stats", ms, {4, 5, 6}); }
int mg_site_stats(mg_ctx *c, float *ms) { return stats(c, "mg_site_stats", ms, {7, 8}); }
int mg_pairs_stats(mg_ctx *c, float *ms) { return stats(c, "mg_pairs_stats", ms, {9, 10}); }
int mg_sample_stats(mg_ctx *c, float *ms) { return stats(c, "mg_sample_stats", ms, {11}); }
int mg_cohort_prior_stats(mg_ctx *c, float *ms) { return stats(c, "mg_cohort_prior_stats", ms, {12}); }
int mg_pl_stats(mg_ctx *c, float *ms) { return stats(c, "mg_pl_stats", ms, {13}); }
// every value of every plane's slice is written: 7
int mg_phred_likelihoods(mg_ctx *c, size_t n, uint32_t planes, const uint32_t *cov, const uint32_t *vao, const uint64_t *var_gt_off, float, int, int, int32_t cap, int32_t *pl_out)
{
    touch(cov, planes * vao[n]);
    say(c, "mg_phred_likelihoods n=%zu planes=%u cap=%d", n, planes, (int)cap);
    for (size_t i = 0; i < planes * var_gt_off[n]; ++i) pl_out[i] = 7;
    return MG_OK;
}

// the two row makers: record r's row is "\tR<r>\n"; the whole capacity they are given is written first.  The line says what was asked for:
// the entry, the mask and the field bits
static int rows(mg_ctx *c, const char *name, const mg_cells &x, char *out, size_t cap, uint64_t *off, uint64_t *need)
{
    const size_t n = x.n_vars, planes = x.n_planes, lists = x.fields ? ((const uint64_t *)x.var_gt_off)[n] : 0;
    touch((const int32_t *)x.gt1, planes * n);
    if (x.fields) touch((const uint32_t *)x.var_allele_off, n + 1);
    if (x.fields & MG_CELLS_GP) touch((const double *)x.probs, planes * lists), touch((const uint8_t *)x.status, planes * n);
    else if (x.probs || x.status) abort(); // (no GP: its arrays are not given)
    for (size_t i = 0; i < ((x.fields & MG_CELLS_PL) ? planes * lists : 0); ++i)
        if (((const int32_t *)x.pl)[i] != 7) abort(); // (what mg_phred_likelihoods left)
    say(c, "%s mask=%d fields=%u n=%zu planes=%zu cap=%zu cov=%d", name, x.use_mask, x.fields, n, planes, cap, (int)(x.cov != nullptr));
    if (cap) memset(out, 'x', cap);
    if (c->first_need && !c->limit_said) {
        c->limit_said = true;
        *need = c->first_need;
        return MG_ERR_LIMIT;
    }
    c->limit_said = false;
    std::string text;
    for (size_t r = 0; r < n; ++r) {
        off[r] = text.size();
        text += "\tR" + std::to_string(r) + "\n";
    }
    off[n] = *need = text.size();
    if (text.size() > cap) return MG_ERR_LIMIT;
    memcpy(out, text.data(), text.size());
    return MG_OK;
}
int mg_format_calls(mg_ctx *c, const mg_cells *x, char *out, size_t cap, uint64_t *off, uint64_t *need) { return rows(c, "mg_format_calls", *x, out, cap, off, need); }
int mg_encode_calls_bcf(mg_ctx *c, const mg_cells *x, const mg_bcf_keys *keys, uint8_t *out, size_t cap, uint64_t *off, uint64_t *need)
{
    if ((x->fields & MG_CELLS_PL) && keys->pl != 8) abort(); // (small_header's ninth ID)
    return rows(c, "mg_encode_calls_bcf", *x, (char *)out, cap, off, need);
}
int mg_site_counts(mg_ctx *c, size_t n, uint32_t planes, int, const int32_t *gt1, const int32_t *, const int32_t *, int use_mask, int32_t, const uint32_t *vao, int accumulate,
                   uint32_t *ac, uint32_t *ns)
{
    touch(gt1, planes * n);
    say(c, "mg_site_counts n=%zu planes=%u mask=%d acc=%d", n, planes, use_mask, accumulate);
    for (size_t i = 0; i < vao[n]; ++i) ac[i] = 3;
    for (size_t i = 0; i < n; ++i) ns[i] = planes;
    return MG_OK;
}
int mg_format_site_info(mg_ctx *c, size_t n, const uint32_t *ac, const uint32_t *ns, const uint32_t *vao, char *out, size_t cap, uint64_t *off, uint64_t *need)
{
    touch(ac, vao[n]);
    say(c, "mg_format_site_info n=%zu cap=%zu", n, cap);
    if (cap) memset(out, 'x', cap);
    std::string text;
    for (size_t r = 0; r < n; ++r) {
        off[r] = text.size();
        text += "NS=" + std::to_string(ns[r]);
    }
    off[n] = *need = text.size();
    if (text.size() > cap) return MG_ERR_LIMIT;
    memcpy(out, text.data(), text.size());
    return MG_OK;
}
int mg_pack_dosage(mg_ctx *c, size_t n, uint32_t planes, int, const int32_t *gt1, const int32_t *, const int32_t *, int, int32_t, const uint32_t *, uint64_t *planes_out)
{
    touch(gt1, planes * n);
    say(c, "mg_pack_dosage n=%zu planes=%u", n, planes);
    for (size_t i = 0; i < planes * 3 * ((n + 63) / 64); ++i) planes_out[i] = 0xABC;
    return MG_OK;
}
int mg_pair_counts(mg_ctx *c, size_t n_words, const uint64_t *planes_a, uint32_t n_a, const uint64_t *planes_b, uint32_t n_b, int accumulate, uint64_t *counts)
{
    touch(planes_a, n_a * 3 * n_words);
    say(c, "mg_pair_counts words=%zu a=%u b=%u other=%d acc=%d", n_words, n_a, n_b, (int)(planes_b != nullptr), accumulate);
    for (size_t i = 0; i < (size_t)n_a * n_b * 9; ++i) counts[i] += 1;
    return MG_OK;
}
int mg_sample_counts(mg_ctx *c, size_t n, uint32_t planes, int, const int32_t *gt1, const int32_t *, const int32_t *, int, int32_t, const uint8_t *status, const uint32_t *cov,
                     const uint32_t *vao, const uint8_t *, int accumulate, uint64_t *counts)
{
    touch(gt1, planes * n), touch(status, planes * n), touch(cov, planes * vao[n]);
    say(c, "mg_sample_counts n=%zu planes=%u acc=%d", n, planes, accumulate);
    for (size_t i = 0; i < (size_t)planes * MG_SAMPLE_SLOTS; ++i) counts[i] += 1;
    return MG_OK;
}
// every record: all planes usable; its slot a holds a heterozygotes and one homozygote
int mg_site_geno_counts(mg_ctx *c, size_t n, uint32_t planes, int, const int32_t *gt1, const int32_t *, const int32_t *, int use_mask, int32_t, const uint32_t *vao,
                        int accumulate, uint32_t *n_out, uint32_t *het, uint32_t *hom)
{
    touch(gt1, planes * n);
    say(c, "mg_site_geno_counts n=%zu planes=%u mask=%d acc=%d", n, planes, use_mask, accumulate);
    for (size_t v = 0; v < n; ++v) {
        n_out[v] = planes;
        for (uint32_t s = vao[v]; s < vao[v + 1]; ++s) het[s] = s - vao[v], hom[s] = 1;
    }
    return MG_OK;
}
int mg_hwe_exact(mg_ctx *c, size_t n_items, const uint32_t *n, const uint32_t *het, const uint32_t *hom, double *hwe, double *exc)
{
    touch(n, n_items), touch(het, n_items), touch(hom, n_items);
    say(c, "mg_hwe_exact items=%zu", n_items);
    for (size_t i = 0; i < n_items; ++i) hwe[i] = 0.5, exc[i] = 0.25;
    return MG_OK;
}
int mg_hwe_stats(mg_ctx *c, float *ms) { return stats(c, "mg_hwe_stats", ms, {14, 15}); }
// every word is written: record v's are v, planes and use_mask
int mg_pack_site_dosage(mg_ctx *c, size_t n, uint32_t planes, int, const int32_t *gt1, const int32_t *, const int32_t *, int use_mask, int32_t, const uint32_t *vao,
                        uint64_t *sites_out)
{
    touch(gt1, planes * n), touch(vao, n + 1);
    say(c, "mg_pack_site_dosage n=%zu planes=%u mask=%d", n, planes, use_mask);
    for (size_t v = 0; v < n; ++v) sites_out[v] = v, sites_out[n + v] = planes, sites_out[2 * n + v] = (uint64_t)use_mask;
    return MG_OK;
}
int mg_ld_stats(mg_ctx *c, float *ms) { return stats(c, "mg_ld_stats", ms, {16, 17}); }
} // extern "C"

// ---- a pass over hand-made batches on fake devices ------------------------------------------------------------------------------------------
using Log = std::vector<std::string>;
static std::string scratch = ".";
static std::string slurp(const std::string &path)
{
    std::ifstream in(path, std::ios::binary);
    CHECK(in.good());
    std::ostringstream s;
    s << in.rdbuf();
    return s.str();
}
static Log only(const Log &log, std::initializer_list<const char *> prefixes) // the lines that start with one of them
{
    Log out;
    for (const std::string &l : log)
        for (const char *p : prefixes)
            if (l.compare(0, strlen(p), p) == 0) {
                out.push_back(l);
                break;
            }
    return out;
}
static bool same_kind(const CallTimes::Kind &k, std::initializer_list<double> ms, std::initializer_list<size_t> calls)
{
    double m[3] = {0, 0, 0};
    size_t n[3] = {0, 0, 0};
    std::copy(ms.begin(), ms.end(), m);
    std::copy(calls.begin(), calls.end(), n);
    return std::equal(m, m + 3, k.ms) && std::equal(n, n + 3, k.calls);
}
static const std::initializer_list<double> no_ms = {};
static const std::initializer_list<size_t> no_calls = {};

static std::deque<Pass> passes; // (a batch points into its pass: the contigs its blocks lie on)
static Pass &new_pass(const BatchRules &rules)
{
    passes.emplace_back(rules);
    return passes.back();
}
static Closed closed_of(Pass &p)
{
    p.b.flush();
    CHECK(p.closed.size() == 1);
    return std::move(p.closed[0]);
}
//                                k  haploid dense samples iso    host   sample records
static const BatchRules dense2{35, false, true, 2, false, false, false, 1000}, kept2{35, false, false, 2, false, false, false, 1000};

// two lone records (for mg_call_isolated) and one general block of two; with `three`, the second record of either kind has three alleles
static Closed mixed_batch(size_t n_samples, bool three)
{
    BatchRules r = dense2;
    r.dense_gt = n_samples <= SPARSE_GT_SAMPLES;
    r.n_samples_kept = n_samples;
    r.iso_path = true;
    const std::vector<std::string> alts = three ? std::vector<std::string>{"G", "T"} : std::vector<std::string>{"G"};
    Pass &p = new_pass(r);
    p.add(block_of(35, {var("c1", 100, "A", {"G"}, n_samples)}));
    p.add(block_of(35, {var("c1", 300, "C", alts, n_samples)}));
    p.add(block_of(35, {var("c1", 500, "A", {"G"}, n_samples), var("c1", 510, "C", alts, n_samples)}));
    return closed_of(p);
}
// three general blocks of one, two and one records, every record kept
static Closed three_blocks(unsigned k = 35)
{
    BatchRules r = kept2;
    r.k = k;
    Pass &p = new_pass(r);
    p.add(block_of((int)k, {var("c1", 200, "A", {"G"})}));
    p.add(block_of((int)k, {var("c1", 400, "A", {"G"}), var("c1", 405, "A", {"G"})}));
    p.add(block_of((int)k, {var("c1", 600, "A", {"G"})}));
    return closed_of(p);
}

struct Scene {
    std::vector<Device> devs; // (first: the last to go)
    Options o;
    PassOut to;
    MergedFormat fmt;
    PriorsFile priors;
    CallTimes total;
    PartFile merged, counts, cov;
    explicit Scene(size_t n_devices = 1) : devs(n_devices)
    {
        for (Device &d : devs) d.ctx = new mg_ctx;
    }
    mg_ctx &ctx(size_t d = 0) { return *devs[d].ctx; }
    void per_sample(size_t planes)
    {
        for (size_t p = 0; p < planes; ++p) {
            to.per_sample.emplace_back();
            to.per_sample.back().open(scratch + "/call_worker_check.s" + std::to_string(p), PartFile::SCRATCH);
        }
    }
    void with_merged()
    {
        merged.open(scratch + "/call_worker_check.merged", PartFile::SCRATCH);
        to.merged = &merged;
        to.merged_fixed = true;
    }
    std::string sample_text(size_t p)
    {
        fflush(to.per_sample[p].f); // (a pass that ended in an error did not)
        return slurp(to.per_sample[p].path);
    }
    // after_submit(i), when set: on the submitting thread, when submit has returned for batch i
    void run(uint32_t planes, size_t n_samples, std::vector<Closed> batches, const std::function<void(size_t)> &after_submit = nullptr)
    {
        PanelPass pass(devs, o, planes, to, n_samples, fmt, priors, total);
        for (size_t i = 0; i < batches.size(); ++i) {
            Closed &c = batches[i];
            pass.submit(std::move(c.recs), std::move(c.iso), std::move(c.gen));
            if (after_submit) after_submit(i);
        }
        pass.finish();
    }
    void run(uint32_t planes, size_t n_samples, Closed batch)
    {
        std::vector<Closed> one;
        one.push_back(std::move(batch));
        run(planes, n_samples, std::move(one));
    }
};
struct CerrCapture { // what the worker says on stderr meanwhile
    std::ostringstream text;
    std::streambuf *was = std::cerr.rdbuf(text.rdbuf());
    ~CerrCapture() { std::cerr.rdbuf(was); }
};

// ---- 1. call_grown ---------------------------------------------------------------------------------------------------------------------------
static void check_call_grown()
{
    {
        std::vector<char> buf(10);
        std::vector<size_t> seen;
        const int rc = call_grown(buf, [&](uint64_t *need) {
            seen.push_back(buf.size());
            *need = 37;
            return buf.size() < 37 ? MG_ERR_LIMIT : MG_OK;
        });
        CHECK(rc == MG_OK && buf.size() == 37 && same<size_t>(seen, {10, 37})); // grown to exactly the need, called once more
    }
    for (uint64_t said : {(uint64_t)10, (uint64_t)3, (uint64_t)0}) { // a limit the buffer already meets: returned at once
        std::vector<char> buf(10);
        int calls = 0;
        const int rc = call_grown(buf, [&](uint64_t *need) {
            ++calls;
            *need = said;
            return MG_ERR_LIMIT;
        });
        CHECK(rc == MG_ERR_LIMIT && calls == 1 && buf.size() == 10);
    }
    for (int code : {MG_OK, MG_ERR_HIP, MG_ERR_ARG, MG_ERR_NOMEM}) { // any other code is passed through, whatever the need says
        std::vector<char> buf(10);
        int calls = 0;
        const int rc = call_grown(buf, [&](uint64_t *need) {
            ++calls;
            *need = 1000;
            return code;
        });
        CHECK(rc == code && calls == 1 && buf.size() == 10);
    }
}

// ---- 2. CallTimes ----------------------------------------------------------------------------------------------------------------------------
static CallTimes some_times(bool with_format, bool with_bcf)
{
    CallTimes t;
    const float pair_ms[2] = {1, 2}, one = 1.5f, half = 0.5f, quarter = 0.25f, three[3] = {1, 2, 3};
    t.pairs.add(pair_ms, 2), t.pairs.add(pair_ms, 2); // two of each, 2 ms and 4 ms
    t.pairs.ms[1] += 2, t.pairs.calls[1] += 2;        // (the pair pass: counts alone) -> 4 counts, 6 ms
    t.sample.add(&one, 1), t.sample.add(&one, 1);
    for (int i = 0; i < 4; ++i) t.prior.add(&half, 1);
    t.estimate.add(&quarter, 1);
    for (int w = 0; w < 2 && with_format; ++w) {
        for (int i = 0; i < 3; ++i) t.format.ms[i] += three[i];
        ++t.format.calls[0];
    }
    for (int i = 0; i < 3 && with_bcf; ++i) t.bcf.ms[i] += 2 * three[i];
    t.bcf.calls[0] += with_bcf;
    t.site.ms[0] = 4, t.site.ms[1] = 6, t.site.calls[0] = t.site.calls[1] = 2;
    t.gt_bytes = 100;
    return t;
}
static void check_call_times()
{
    CallTimes a = some_times(true, false);
    a += some_times(false, true);
    CHECK(same_kind(a.pairs, {4, 12}, {4, 8}) && same_kind(a.sample, {6}, {4}) && same_kind(a.prior, {4}, {8}) && same_kind(a.estimate, {0.5}, {2}));
    CHECK(same_kind(a.format, {2, 4, 6}, {2}) && same_kind(a.bcf, {2, 4, 6}, {1}) && same_kind(a.site, {8, 12}, {4, 4}) && a.gt_bytes == 200);

    CHECK(!g_timers.on && a.report().empty()); // the timers off: nothing
    a.add_to_timers();
    CHECK(g_timers.acc.empty());
    g_timers.on = true;
    CHECK(CallTimes().report().empty()); // the counts zero: nothing
    CHECK(some_times(true, false).report() == "[malva-geno] pairs: 2 mg_pack_dosage, 4 mg_pair_counts, device ms per call: pack 1.000 count 1.500\n"
                                              "[malva-geno] sample-stats: 2 mg_sample_counts, device ms per call: count 1.500\n"
                                              "[malva-geno] cohort-priors: 4 mg_genotype_cohort, device ms per call: 0.500\n"
                                              "[malva-geno] cohort-priors: 1 mg_estimate_priors, device ms per call: 0.250\n"
                                              "[malva-geno] merged: 2 mg_format_calls, device ms per call: length 1.000 scan 2.000 write 3.000\n"
                                              "[malva-geno] merged: 2 mg_site_counts, 2 mg_format_site_info, device ms per call: count 2.000 info 3.000\n");
    // BCF: mg_site_counts has a line of its own, behind the encoder's
    CHECK(some_times(false, true).report() == "[malva-geno] pairs: 2 mg_pack_dosage, 4 mg_pair_counts, device ms per call: pack 1.000 count 1.500\n"
                                              "[malva-geno] sample-stats: 2 mg_sample_counts, device ms per call: count 1.500\n"
                                              "[malva-geno] cohort-priors: 4 mg_genotype_cohort, device ms per call: 0.500\n"
                                              "[malva-geno] cohort-priors: 1 mg_estimate_priors, device ms per call: 0.250\n"
                                              "[malva-geno] merged: 1 mg_encode_calls_bcf, device ms per call: length 2.000 scan 4.000 write 6.000\n"
                                              "[malva-geno] merged: 2 mg_site_counts, device ms per call: count 2.000\n");
    {
        CallTimes t; // the pair pass alone counted (a cohort in groups whose batches made no pack call is not a case; the guard is): pack prints 0
        t.pairs.ms[1] = 3, t.pairs.calls[1] = 2;
        CHECK(t.report() == "[malva-geno] pairs: 0 mg_pack_dosage, 2 mg_pair_counts, device ms per call: pack 0.000 count 1.500\n");
        t = CallTimes();
        t.pairs.ms[0] = 3, t.pairs.calls[0] = 2; // no count: no line
        t.site.calls[0] = 2;                     // counts without a row maker: no line
        CHECK(t.report().empty());
        t.format.calls[0] = 1; // text, counts but no mg_format_site_info (the groups' counts went to a file, the paste pass made none): the format line alone
        CHECK(t.report() == "[malva-geno] merged: 1 mg_format_calls, device ms per call: length 0.000 scan 0.000 write 0.000\n");
    }
    // report() leaves the timers alone; add_to_timers() puts the sums under their labels, in seconds, under the same conditions
    CHECK(g_timers.acc.empty());
    some_times(true, false).add_to_timers();
    some_times(false, true).add_to_timers();
    {
        CallTimes t;
        t.add_to_timers();                       // the counts zero: nothing
        t.pairs.ms[0] = 3, t.pairs.calls[0] = 2; // no count: nothing
        t.site.ms[0] = 5, t.site.calls[0] = 2;   // (the site counts have no label of their own)
        t.add_to_timers();
    }
    CHECK(g_timers.acc.at("pairs: pack and count kernels (device)") == 2 * 0.008 && g_timers.acc.at("sample table: count kernel (device)") == 2 * 0.003);
    CHECK(g_timers.acc.at("cohort priors: kernel (device)") == 2 * 0.002 && g_timers.acc.at("cohort priors: estimate kernel (device)") == 2 * 0.00025);
    CHECK(g_timers.acc.at("merged: format kernels (device)") == 0.012 + 0.0 && g_timers.acc.at("merged: encode kernels (device)") == 0.012 && g_timers.acc.size() == 6);
    g_timers.on = false;
    g_timers.acc.clear();
}

// ---- 3. one sample ---------------------------------------------------------------------------------------------------------------------------
static void check_one_sample()
{
    {
        Scene s;
        s.per_sample(1);
        s.run(0, 2, mixed_batch(2, false));
        CHECK(s.ctx().log == Log({"mg_call_isolated n=2 cov+0 g1+0 probs+-1", "mg_cover_blocks blocks=1 n=2 samples=2 dense=1 sparse=0", "mg_genotype n=2 cov+0 g1+0 probs+-1 id=0"}));
        CHECK(s.sample_text(0) == "c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t0/1:10\n"
                                  "c1\t301\t.\tC\tG\t.\tPASS\t.\tGT:GQ\t0/1:11\n"
                                  "c1\t501\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:50\n"
                                  "c1\t511\t.\tC\tG\t.\tPASS\t.\tGT:GQ\t1/1:51\n");
        CHECK(s.total.gt_bytes == 8); // two records, two samples, a word each
    }
    {
        Scene s; // 65 samples: the sparse form -- three offsets and every sample of both records (0|1 is not the default word)
        s.per_sample(1);
        s.run(0, 65, mixed_batch(65, false));
        CHECK(s.ctx().log == Log({"mg_call_isolated n=2 cov+0 g1+0 probs+-1", "mg_cover_blocks blocks=1 n=2 samples=65 dense=0 sparse=1", "mg_genotype n=2 cov+0 g1+0 probs+-1 id=0"}));
        CHECK(s.total.gt_bytes == 4 * 3 + 6 * 130);
    }
}

// ---- 4. three planes, records of 2 and 3 alleles ------------------------------------------------------------------------------------------------
static void check_three_planes()
{
    const Log lone_calls{"mg_cohort_select 0", "mg_call_isolated n=2 cov+0 g1+0 probs+0",  "mg_cohort_select 1", "mg_call_isolated n=2 cov+5 g1+2 probs+9",
                         "mg_cohort_select 2", "mg_call_isolated n=2 cov+10 g1+4 probs+18"};
    const Log genotypes{"mg_genotype n=2 cov+0 g1+0 probs+0 id=0", "mg_genotype n=2 cov+5 g1+2 probs+9 id=0", "mg_genotype n=2 cov+10 g1+4 probs+18 id=0"};
    for (size_t n_samples : {2, 65}) {
        Scene s;
        s.o.verbose = true; // (the likelihood lists: 3 + 6 genotype slots per plane)
        s.ctx().n_planes = 3;
        s.per_sample(3);
        s.run(3, n_samples, mixed_batch(n_samples, true));
        Log want = lone_calls;
        want.push_back(n_samples == 2 ? "mg_cover_blocks_cohort blocks=1 n=2 samples=2 dense=1 sparse=0" : "mg_cover_blocks_cohort blocks=1 n=2 samples=65 dense=0 sparse=1");
        want.insert(want.end(), genotypes.begin(), genotypes.end());
        CHECK(s.ctx().log == want);
        // the middle plane reads what the middle calls wrote
        CHECK(s.sample_text(1) == "c1\t101\t.\tA\tG\t.\tPASS\tCOVS=20,21;GTS=0/0:0.500000,0/1:0.500000,1/1:0.500000\tGT:GQ\t0/1:20\n"
                                  "c1\t301\t.\tC\tG,T\t.\tPASS\tCOVS=22,23,24;GTS=0/0:0.500000,0/1:0.500000,0/2:0.500000,1/1:0.500000,1/2:0.500000,2/2:0.500000\tGT:GQ\t0/1:21\n"
                                  "c1\t501\t.\tA\tG\t.\tPASS\tCOVS=200,201;GTS=0/0:0.250000,0/1:0.250000,1/1:0.250000\tGT:GQ\t1/1:60\n"
                                  "c1\t511\t.\tC\tG,T\t.\tPASS\tCOVS=202,203,204;GTS=0/0:0.250000,0/1:0.250000,0/2:0.250000,1/1:0.250000,1/2:0.250000,2/2:0.250000\tGT:GQ\t1/1:61\n");
        CHECK(s.sample_text(0).find("COVS=10,11;") != std::string::npos && s.sample_text(2).find("COVS=302,303,304;") != std::string::npos);
    }
}

// ---- 5. the host enumerator -------------------------------------------------------------------------------------------------------------------
static void check_host_fallback()
{
    {
        Scene s; // the device hands back the second record of the middle block: that block, once, and a lookup per plane at its first allele slot
        s.o.verbose = true;
        s.ctx().n_planes = 2;
        s.ctx().flagged = {2};
        s.per_sample(2);
        CerrCapture err;
        s.run(2, 2, three_blocks());
        CHECK(s.ctx().log == Log({"mg_cover_blocks_cohort blocks=3 n=4 samples=2 dense=1 sparse=0", "mg_cohort_select 0", "mg_lookup_cover plane=0 cov+2 alleles=4", "mg_cohort_select 1",
                                  "mg_lookup_cover plane=1 cov+10 alleles=4", "mg_genotype n=4 cov+0 g1+0 probs+0 id=0", "mg_genotype n=4 cov+8 g1+4 probs+12 id=0"}));
        CHECK(err.text.str() == "[malva-geno] 1 block(s) enumerated on the host\n");
        CHECK(s.sample_text(1) == "c1\t201\t.\tA\tG\t.\tPASS\tCOVS=200,201;GTS=0/0:0.250000,0/1:0.250000,1/1:0.250000\tGT:GQ\t1/1:60\n"
                                  "c1\t401\t.\tA\tG\t.\tPASS\tCOVS=70,71;GTS=0/0:0.250000,0/1:0.250000,1/1:0.250000\tGT:GQ\t1/1:61\n"
                                  "c1\t406\t.\tA\tG\t.\tPASS\tCOVS=72,73;GTS=0/0:0.250000,0/1:0.250000,1/1:0.250000\tGT:GQ\t1/1:62\n"
                                  "c1\t601\t.\tA\tG\t.\tPASS\tCOVS=206,207;GTS=0/0:0.250000,0/1:0.250000,1/1:0.250000\tGT:GQ\t1/1:63\n");
    }
    {
        Scene s; // a record the batch let go of (tier 1 is sure to take it) comes back all the same
        s.ctx().flagged = {0};
        s.per_sample(1);
        Pass &p = new_pass(dense2);
        p.add(block_of(35, {var("c1", 100, "A", {"G"})}));
        Closed c = closed_of(p);
        CHECK(same<int32_t>(c.gen.var_slot, {-1}));
        std::string what;
        try {
            s.run(0, 2, std::move(c));
        } catch (const std::runtime_error &e) {
            what = e.what();
        }
        CHECK(what == "internal: the device handed back a record tier 1 should have taken");
    }
    for (int why = 0; why < 3; ++why) { // a record of more than 127 alleles, k beyond the packed forms, MALVA_GENO_HOST_ENUM: every block, and no cover call
        Scene s;
        s.per_sample(1);
        Closed c = three_blocks(why == 1 ? MG_MAX_PACKED_K + 1 : 35);
        if (why == 0) c.gen.wide_alleles = true;
        if (why == 1) s.o.k = MG_MAX_PACKED_K + 1;
        if (why == 2) setenv("MALVA_GENO_HOST_ENUM", "1", 1);
        CerrCapture err;
        s.run(0, 2, std::move(c));
        unsetenv("MALVA_GENO_HOST_ENUM");
        CHECK(s.ctx().log == Log({"mg_lookup_cover plane=0 cov+0 alleles=2", "mg_lookup_cover plane=0 cov+2 alleles=4", "mg_lookup_cover plane=0 cov+6 alleles=2",
                                  "mg_genotype n=4 cov+0 g1+0 probs+-1 id=0"}));
        CHECK(err.text.str() == "[malva-geno] 3 block(s) enumerated on the host\n");
    }
    {
        Scene s; // k AT the packed forms' limit: the device
        s.o.k = MG_MAX_PACKED_K;
        s.per_sample(1);
        s.run(0, 2, three_blocks(MG_MAX_PACKED_K));
        CHECK(s.ctx().log == Log({"mg_cover_blocks blocks=3 n=4 samples=2 dense=1 sparse=0", "mg_genotype n=4 cov+0 g1+0 probs+-1 id=0"}));
    }
}

// ---- 6. --cohort-priors ------------------------------------------------------------------------------------------------------------------------
static void check_cohort_priors()
{
    const Log lone_calls{"mg_cohort_select 0", "mg_call_isolated n=2 cov+0 g1+0 probs+-1", "mg_cohort_select 1", "mg_call_isolated n=2 cov+4 g1+2 probs+-1"};
    const char *cover = "mg_cover_blocks_cohort blocks=1 n=2 samples=2 dense=1 sparse=0";
    const uint32_t vao[3] = {0, 2, 4};
    const float f0[4] = {0.5f, 0.25f, 0.5f, 0.25f};
    {
        Scene s; // one group: per batch kind ONE mg_genotype_cohort with the option's iterations, and no mg_genotype
        s.o.priors.on = true;
        s.ctx().n_planes = 2;
        s.per_sample(2);
        s.priors.open(scratch + "/call_worker_check.priors");
        s.run(2, 2, mixed_batch(2, false));
        Log want = lone_calls;
        want.insert(want.end(), {"mg_genotype_cohort n=2 planes=2 iters=5 weight=1 freq_copy=0 probs=0", "mg_cohort_prior_stats", cover,
                                 "mg_genotype_cohort n=2 planes=2 iters=5 weight=1 freq_copy=0 probs=0", "mg_cohort_prior_stats"});
        CHECK(s.ctx().log == want);
        CHECK(same_kind(s.total.prior, {24}, {2}));
        CHECK(s.sample_text(1) == "c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t0/0:80\n" "c1\t301\t.\tC\tG\t.\tPASS\t.\tGT:GQ\t0/0:81\n"
                                  "c1\t501\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t0/0:80\n" "c1\t511\t.\tC\tG\t.\tPASS\t.\tGT:GQ\t0/0:81\n");
        s.priors.close();
        CHECK(slurp(s.priors.part) == std::string(priors_header()) + "c1\t101\t.\tA\tG\t0.25\t0.125\t99\n" "c1\t301\t.\tC\tG\t0.25\t0.125\t99\n"
                                                                     "c1\t501\t.\tA\tG\t0.25\t0.125\t99\n" "c1\t511\t.\tC\tG\t0.25\t0.125\t99\n");
    }
    {
        // the output pass of a cohort in several groups: coverages and the cohort's estimate come from the scratch files -- no lone call, no cover call;
        // mg_genotype_cohort with no iterations, the frequencies a copy of freq_out, and the informative counts a scratch array: the table keeps the file's
        const uint32_t cov[8] = {1, 2, 3, 4, 5, 6, 7, 8}, n_lone[2] = {7, 8}, n_other[2] = {5, 6};
        const float f_t[4] = {0.5f, 0.125f, 0.75f, 0.0625f};
        std::string bytes;
        PartFile cov_file, freq_file;
        cov_file.open(scratch + "/call_worker_check.cov", PartFile::SCRATCH);
        freq_file.open(scratch + "/call_worker_check.freq", PartFile::SCRATCH);
        put_cov_batch(bytes, 0, 2, vao, f0, true, 2, cov);
        put_cov_batch(bytes, 1, 2, vao, f0, true, 2, cov);
        cov_file.write(bytes);
        bytes.clear();
        put_freq_batch(bytes, 0, 2, 4, f_t, n_lone);
        put_freq_batch(bytes, 1, 2, 4, f_t, n_other);
        freq_file.write(bytes);
        cov_file.close(), freq_file.close();
        Scene s;
        s.o.priors.on = true;
        s.ctx().n_planes = 2;
        s.per_sample(2);
        s.priors.open(scratch + "/call_worker_check.priors");
        PriorGroupInput in;
        in.open(cov_file.path, freq_file.path, 2);
        s.to.prior_in = &in;
        s.run(2, 2, mixed_batch(2, false));
        CHECK(s.ctx().log == Log({"mg_genotype_cohort n=2 planes=2 iters=0 weight=1 freq_copy=1 probs=0", "mg_cohort_prior_stats",
                                  "mg_genotype_cohort n=2 planes=2 iters=0 weight=1 freq_copy=1 probs=0", "mg_cohort_prior_stats"}));
        s.priors.close();
        CHECK(slurp(s.priors.part) == std::string(priors_header()) + "c1\t101\t.\tA\tG\t0.25\t0.125\t7\n" "c1\t301\t.\tC\tG\t0.25\t0.0625\t8\n"
                                                                     "c1\t501\t.\tA\tG\t0.25\t0.125\t5\n" "c1\t511\t.\tC\tG\t0.25\t0.0625\t6\n");
    }
    {
        Scene s; // the coverage pass: up to the coverages, which it writes as put_cov_batch makes them, and nothing else -- no genotype call, no text
        s.o.priors.on = true;
        s.ctx().n_planes = 2;
        s.per_sample(2);
        s.with_merged();
        s.cov.open(scratch + "/call_worker_check.cov", PartFile::SCRATCH);
        s.to.prior_cov = &s.cov;
        s.to.prior_cov_panel = true;
        s.run(2, 2, mixed_batch(2, false));
        Log want = lone_calls;
        want.push_back(cover);
        CHECK(s.ctx().log == want);
        const uint32_t lone_cov[8] = {10, 11, 12, 13, 20, 21, 22, 23}, other_cov[8] = {100, 101, 102, 103, 200, 201, 202, 203};
        std::string bytes;
        put_cov_batch(bytes, 0, 2, vao, f0, true, 2, lone_cov);
        put_cov_batch(bytes, 1, 2, vao, f0, true, 2, other_cov);
        s.cov.close();
        CHECK(slurp(s.cov.path) == bytes);
        CHECK(s.sample_text(0).empty() && s.sample_text(1).empty() && slurp(s.merged.path).empty());
        CHECK(same_kind(s.total.prior, no_ms, no_calls) && same_kind(s.total.format, no_ms, no_calls));
    }
}

// ---- 7. the merged rows --------------------------------------------------------------------------------------------------------------------------
static BcfHeader small_header()
{
    return bcf_parse_header("##fileformat=VCFv4.2\n##contig=<ID=c1>\n##INFO=<ID=AC,Number=A,Type=Integer>\n##INFO=<ID=AN,Number=1,Type=Integer>\n"
                            "##INFO=<ID=AF,Number=A,Type=Float>\n##INFO=<ID=NS,Number=1,Type=Integer>\n##FORMAT=<ID=GT,Number=1,Type=String>\n"
                            "##FORMAT=<ID=GQ,Number=1,Type=Integer>\n##FORMAT=<ID=GP,Number=G,Type=Float>\n##FORMAT=<ID=PL,Number=G,Type=Integer>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n",
                            true);
}
static void check_merged_rows()
{
    const std::initializer_list<const char *> row_calls = {"mg_format", "mg_encode", "mg_bcf", "mg_site"};
    struct Form {
        bool bcf, gp, min_gq;
        const char *name;
        size_t guess; // two records of two planes: 2 (2 * 10 + 1); with --gp 2 (2 + 9 * 6) more as text, 2 (2 + 4 * 6) as BCF
    };
    const Form forms[] = {{false, false, false, "mg_format_calls mask=0 fields=0", 42},     {false, false, true, "mg_format_calls mask=1 fields=0", 42},
                          {false, true, false, "mg_format_calls mask=0 fields=1", 154},     {false, true, true, "mg_format_calls mask=1 fields=1", 154},
                          {true, false, false, "mg_encode_calls_bcf mask=0 fields=0", 42},  {true, false, true, "mg_encode_calls_bcf mask=1 fields=0", 42},
                          {true, true, false, "mg_encode_calls_bcf mask=0 fields=1", 94},   {true, true, true, "mg_encode_calls_bcf mask=1 fields=1", 94}};
    for (const Form &f : forms) {
        Scene s;
        s.o.gp = f.gp, s.o.use_min_gq = f.min_gq, s.o.min_gq = 20;
        s.fmt.bcf_out = f.bcf, s.fmt.bcf_direct = true, s.fmt.bcf_hdr = small_header();
        s.ctx().n_planes = 2;
        s.ctx().first_need = 1000; // the first answer of every batch kind: a need; the second call sees a buffer of exactly that size
        s.with_merged();
        s.run(2, 2, mixed_batch(2, false));
        const std::string first = std::string(f.name) + " n=2 planes=2 cap=" + std::to_string(f.guess) + " cov=0", second = std::string(f.name) + " n=2 planes=2 cap=1000 cov=0";
        const char *read_stats = f.bcf ? "mg_bcf_stats" : "mg_format_stats";
        CHECK(only(s.ctx().log, row_calls) == Log({first, second, read_stats, first, second, read_stats})); // the lone records', then the others'
        if (f.bcf) CHECK(same_kind(s.total.bcf, {8, 10, 12}, {2}) && same_kind(s.total.format, no_ms, no_calls));
        else CHECK(same_kind(s.total.format, {2, 4, 6}, {2}) && same_kind(s.total.bcf, no_ms, no_calls));
        s.merged.close();
        const std::string fixed = f.gp ? "\t.\tPASS\t.\tGT:GQ:GP\t" : "\t.\tPASS\t.\tGT:GQ\t";
        if (!f.bcf)
            CHECK(slurp(s.merged.path) == "c1\t101\t.\tA\tG" + fixed + "R0\n" + "c1\t301\t.\tC\tG" + fixed + "R1\n" + "c1\t501\t.\tA\tG" + fixed + "R0\n" + "c1\t511\t.\tC\tG" + fixed + "R1\n");
        else CHECK(slurp(s.merged.path).size() > 4 * 4);
    }
    // --pl: one mg_phred_likelihoods over both planes per batch kind, in front of the rows; the row makers under MG_CELLS_PL with and without GP and the mask.
    // The guess: 42, with PL 2 (2 + 4 * 6) more as text and 2 (2 + 2 * 6) as BCF, with GP what GP adds
    struct PlForm {
        bool bcf, gp, min_gq;
        const char *name;
        size_t guess;
    };
    const PlForm pl_forms[] = {{false, false, false, "mg_format_calls mask=0 fields=2", 94},    {false, true, true, "mg_format_calls mask=1 fields=3", 206},
                               {true, false, true, "mg_encode_calls_bcf mask=1 fields=2", 70},  {true, true, false, "mg_encode_calls_bcf mask=0 fields=3", 122}};
    for (const PlForm &f : pl_forms) {
        Scene s;
        s.o.pl = true, s.o.pl_cap = 99, s.o.gp = f.gp, s.o.use_min_gq = f.min_gq, s.o.min_gq = 20;
        s.fmt.bcf_out = f.bcf, s.fmt.bcf_direct = true, s.fmt.bcf_hdr = small_header();
        s.ctx().n_planes = 2;
        s.ctx().first_need = 1000;
        s.with_merged();
        s.run(2, 2, mixed_batch(2, false));
        const std::string first = std::string(f.name) + " n=2 planes=2 cap=" + std::to_string(f.guess) + " cov=0", second = std::string(f.name) + " n=2 planes=2 cap=1000 cov=0";
        const char *read_stats = f.bcf ? "mg_bcf_stats" : "mg_format_stats", *pl_call = "mg_phred_likelihoods n=2 planes=2 cap=99";
        CHECK(only(s.ctx().log, {"mg_format", "mg_encode", "mg_bcf", "mg_site", "mg_phred", "mg_pl_"}) ==
              Log({pl_call, "mg_pl_stats", pl_call, "mg_pl_stats", first, second, read_stats, first, second, read_stats})); // both kinds' likelihoods, then both kinds' rows
        CHECK(same_kind(s.total.pl, {26}, {2}));
        CHECK(s.fmt.n_fields(s.o) == (f.gp ? 4u : 3u));
        s.merged.close();
        const std::string fixed = f.gp ? "\t.\tPASS\t.\tGT:GQ:GP:PL\t" : "\t.\tPASS\t.\tGT:GQ:PL\t";
        if (!f.bcf)
            CHECK(slurp(s.merged.path) == "c1\t101\t.\tA\tG" + fixed + "R0\n" + "c1\t301\t.\tC\tG" + fixed + "R1\n" + "c1\t501\t.\tA\tG" + fixed + "R0\n" + "c1\t511\t.\tC\tG" + fixed + "R1\n");
        else CHECK(slurp(s.merged.path).size() > 4 * 4);
    }
    {
        CallTimes t; // the likelihoods' line of the report and their label
        const float ms = 3;
        t.pl.add(&ms, 1), t.pl.add(&ms, 1);
        g_timers.on = true;
        CHECK(t.report() == "[malva-geno] merged: 2 mg_phred_likelihoods, device ms per call: 3.000\n");
        t.add_to_timers();
        CHECK(g_timers.acc.size() == 1 && g_timers.acc.at("merged: likelihood kernel (device)") == 0.006);
        g_timers.on = false;
        g_timers.acc.clear();
    }
    for (int where = 0; where < 3; ++where) { // --site-tags: INFO made at once (text, the group is the cohort) | the counts to a file | BCF (INFO made on the host)
        Scene s;
        s.o.site_tags = true;
        s.fmt.bcf_out = where == 2, s.fmt.bcf_direct = true, s.fmt.bcf_hdr = small_header();
        s.ctx().n_planes = 2;
        s.with_merged();
        if (where == 1) {
            s.counts.open(scratch + "/call_worker_check.cnt", PartFile::SCRATCH);
            s.to.site_counts = &s.counts;
        }
        std::vector<uint64_t> sample_table(2 * MG_SAMPLE_SLOTS, 0);
        PairsRun pairs;
        pairs.counts.assign(2 * 2 * 9, 0);
        s.to.pairs = &pairs; // (and the two tables beside them)
        s.to.sample_table = sample_table.data();
        s.run(2, 2, mixed_batch(2, false));
        const char *row = where == 2 ? "mg_encode_calls_bcf mask=0 fields=0 n=2 planes=2 cap=42 cov=0" : "mg_format_calls mask=0 fields=0 n=2 planes=2 cap=42 cov=0", *read_stats = where == 2 ? "mg_bcf_stats" : "mg_format_stats";
        Log kind{row, read_stats, "mg_site_counts n=2 planes=2 mask=0 acc=0", "mg_site_stats"};
        if (where == 0) kind.insert(kind.end(), {"mg_format_site_info n=2 cap=80", "mg_site_stats"});
        Log want = kind;
        want.insert(want.end(), kind.begin(), kind.end());
        CHECK(only(s.ctx().log, row_calls) == want);
        if (where == 0) CHECK(same_kind(s.total.site, {14, 16}, {2, 2}));
        else CHECK(same_kind(s.total.site, {14}, {2}));
        s.merged.close();
        if (where == 0)
            CHECK(slurp(s.merged.path) == "c1\t101\t.\tA\tG\t.\tPASS\tNS=2\tGT:GQ\tR0\n" "c1\t301\t.\tC\tG\t.\tPASS\tNS=2\tGT:GQ\tR1\n"
                                          "c1\t501\t.\tA\tG\t.\tPASS\tNS=2\tGT:GQ\tR0\n" "c1\t511\t.\tC\tG\t.\tPASS\tNS=2\tGT:GQ\tR1\n");
        if (where == 1) {
            CHECK(slurp(s.merged.path) == "c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\tR0\n" "c1\t301\t.\tC\tG\t.\tPASS\t.\tGT:GQ\tR1\n"
                                          "c1\t501\t.\tA\tG\t.\tPASS\t.\tGT:GQ\tR0\n" "c1\t511\t.\tC\tG\t.\tPASS\t.\tGT:GQ\tR1\n");
            const uint32_t record[4] = {2, 2, 3, 3}; // n_alleles, ns, ac[2]
            std::string four;
            for (int r = 0; r < 4; ++r) four.append((const char *)record, sizeof record);
            s.counts.close();
            CHECK(slurp(s.counts.path) == four);
        }
        // the pair table and the sample table: a pack, a count and a sample count per batch kind, into the pass's own arrays
        CHECK(only(s.ctx().log, {"mg_pack", "mg_pair", "mg_sample"}) ==
              Log({"mg_pack_dosage n=2 planes=2", "mg_pair_counts words=1 a=2 b=2 other=0 acc=1", "mg_pairs_stats", "mg_pack_dosage n=2 planes=2",
                   "mg_pair_counts words=1 a=2 b=2 other=0 acc=1", "mg_pairs_stats", "mg_sample_counts n=2 planes=2 acc=1", "mg_sample_stats", "mg_sample_counts n=2 planes=2 acc=1",
                   "mg_sample_stats"}));
        CHECK(same_kind(s.total.pairs, {18, 20}, {2, 2}) && same_kind(s.total.sample, {22}, {2}));
        CHECK(pairs.counts == std::vector<uint64_t>(36, 2) && sample_table == std::vector<uint64_t>(2 * MG_SAMPLE_SLOTS, 2));
    }
}

// ---- 8. the pipeline -------------------------------------------------------------------------------------------------------------------------------
static std::vector<Closed> five_batches()
{
    std::vector<Closed> batches;
    for (int i = 0; i < 5; ++i) {
        Pass &p = new_pass(dense2);
        Variant v = var("c1", 100 + 100 * i, "A", {"G"});
        v.frequencies[0] = (float)i; // (what the fake of mg_genotype knows a batch by)
        p.add(block_of(35, {std::move(v)}));
        batches.push_back(closed_of(p));
    }
    return batches;
}
static Log genotype_ids(const Log &log)
{
    Log ids;
    for (const std::string &l : only(log, {"mg_genotype "})) ids.push_back(l.substr(l.find("id=")));
    return ids;
}
static void check_pipeline()
{
    {
        Scene s(2);
        Sync sync;
        s.ctx(0).sync = s.ctx(1).sync = &sync;
        s.ctx(1).odd = true;
        s.per_sample(1);
        s.with_merged();
        // Never more than two in flight: only the submitting thread adds a batch's 4 bytes to the run's total, as it takes the batch.  When submit
        // has returned for batch i, batches 0 .. i - 2 have been taken -- batch i was not started before -- and no more: batch i - 1 is still in flight
        std::vector<size_t> taken;
        s.run(0, 2, five_batches(), [&](size_t) { taken.push_back(s.total.gt_bytes / 4); });
        CHECK(same<size_t>(taken, {0, 0, 1, 2, 3}));
        CHECK(!sync.timed_out && sync.most_active == 2); // batch i + 1 ran while batch i waited for it: two at once
        CHECK(genotype_ids(s.ctx(0).log) == Log({"id=0", "id=2", "id=4"}) && genotype_ids(s.ctx(1).log) == Log({"id=1", "id=3"})); // job i on device i % 2
        // every odd batch was done before the even batch in front of it: the text leaves in submission order all the same
        CHECK(s.sample_text(0) == "c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:50\n" "c1\t201\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:50\n" "c1\t301\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:50\n"
                                  "c1\t401\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:50\n" "c1\t501\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:50\n");
        s.merged.close();
        CHECK(slurp(s.merged.path) == "c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\tR0\n" "c1\t201\t.\tA\tG\t.\tPASS\t.\tGT:GQ\tR0\n" "c1\t301\t.\tA\tG\t.\tPASS\t.\tGT:GQ\tR0\n"
                                      "c1\t401\t.\tA\tG\t.\tPASS\t.\tGT:GQ\tR0\n" "c1\t501\t.\tA\tG\t.\tPASS\t.\tGT:GQ\tR0\n");
        // the run's times: five batches of one record of two samples (4 bytes of genotype words) and of one mg_format_calls (1, 2 and 3 ms)
        CHECK(s.total.gt_bytes == 20 && same_kind(s.total.format, {5, 10, 15}, {5}));
        CHECK(same_kind(s.total.bcf, no_ms, no_calls) && same_kind(s.total.site, no_ms, no_calls) && same_kind(s.total.pairs, no_ms, no_calls) &&
              same_kind(s.total.sample, no_ms, no_calls) && same_kind(s.total.prior, no_ms, no_calls) && same_kind(s.total.estimate, no_ms, no_calls));
    }
    {
        Scene s(2); // the third batch's mg_genotype fails: its error leaves the pass, and the batches behind it are awaited before their devices go
        s.ctx(0).fail_genotype_at = 2;
        s.per_sample(1);
        std::string what;
        try {
            s.run(0, 2, five_batches());
        } catch (const std::runtime_error &e) {
            what = e.what();
        }
        CHECK(what == "mg_genotype: fake: the device said no");
        CHECK(s.sample_text(0) == "c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:50\n" "c1\t201\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:50\n"); // what came before it was written
    }
}

// ---- 9. the records' site words (--ld, --ibd, --grm) ------------------------------------------------------------------------------------------------
// lone records and general blocks in turn: the output order is neither batch kind's order
static Closed interleaved_batch()
{
    BatchRules r = dense2;
    r.iso_path = true;
    Pass &p = new_pass(r);
    p.add(block_of(35, {var("c1", 100, "A", {"G"})}));
    p.add(block_of(35, {var("c1", 300, "A", {"G"}), var("c1", 310, "C", {"G", "T"})}));
    p.add(block_of(35, {var("c1", 500, "C", {"G", "T"})}));
    p.add(block_of(35, {var("c1", 700, "A", {"G"}), var("c1", 705, "A", {"G"})}));
    p.add(block_of(35, {var("c1", 900, "A", {"G"})}));
    return closed_of(p);
}
static void check_site_words()
{
    struct Want { // a record of the stream: its slot in its batch kind (the fake's first word), its alleles, its first five columns
        uint64_t slot;
        uint32_t n_alleles;
        const char *cols;
    };
    const Want want[] = {{0, 2, "c1\t101\t.\tA\tG"}, {0, 2, "c1\t301\t.\tA\tG"}, {1, 3, "c1\t311\t.\tC\tG,T"}, {1, 3, "c1\t501\t.\tC\tG,T"}, {2, 2, "c1\t701\t.\tA\tG"},
                         {3, 2, "c1\t706\t.\tA\tG"}, {2, 2, "c1\t901\t.\tA\tG"}, // the interleaved batch: lone, two general, lone, two general, lone
                         {0, 2, "c1\t101\t.\tA\tG"}, {1, 3, "c1\t301\t.\tC\tG,T"}, {0, 2, "c1\t501\t.\tA\tG"}, {1, 3, "c1\t511\t.\tC\tG,T"}}; // mixed_batch: two lone, two general
    const char *labels[3] = {"worker: ld words (mg_pack_site_dosage)", "worker: ibd words (mg_pack_site_dosage)", "worker: grm words (mg_pack_site_dosage)"};
    for (int asked = 0; asked < 3; ++asked) // LD asked; IBD without LD; GRM alone
        for (const bool cols : {true, false}) {
            Scene s;
            s.o.use_min_gq = true, s.o.min_gq = 20;
            s.ctx().n_planes = 2;
            PartFile words;
            words.open(scratch + "/call_worker_check.sites", PartFile::SCRATCH);
            s.to.site_words = &words, s.to.site_words_cols = cols;
            s.to.site_words_for = asked == 0 ? PassOut::LD : asked == 1 ? PassOut::IBD : PassOut::GRM;
            std::vector<Closed> batches;
            batches.push_back(interleaved_batch());
            batches.push_back(mixed_batch(2, true));
            std::vector<bool> lone;
            for (const Rec &r : batches[0].recs) lone.push_back(r.isolated);
            CHECK(lone == std::vector<bool>({true, false, false, true, false, false, true}));
            g_timers.on = true;
            s.run(2, 2, std::move(batches));
            g_timers.on = false;
            for (int k = 0; k < 3; ++k) CHECK(g_timers.acc.count(labels[k]) == (k == asked)); // the worker's timer: the asking option's alone
            g_timers.acc.clear();
            // a pack call per batch kind, the lone records' first, over both planes and under the mask
            CHECK(only(s.ctx().log, {"mg_pack", "mg_ld_"}) == Log({"mg_pack_site_dosage n=3 planes=2 mask=1", "mg_ld_stats", "mg_pack_site_dosage n=4 planes=2 mask=1", "mg_ld_stats",
                                                                   "mg_pack_site_dosage n=2 planes=2 mask=1", "mg_ld_stats", "mg_pack_site_dosage n=2 planes=2 mask=1", "mg_ld_stats"}));
            const CallTimes::Kind *kinds[3] = {&s.total.ld, &s.total.ibd, &s.total.grm};
            for (int k = 0; k < 3; ++k) CHECK(k == asked ? same_kind(*kinds[k], {64}, {4}) : same_kind(*kinds[k], no_ms, no_calls)); // four calls of 16 ms
            // the stream: put_site_words over the records in output order -- the fake's words are the slot, the planes and the mask
            std::string bytes;
            for (const Want &w : want) put_site_words(bytes, w.slot, 2, 1, w.n_alleles, cols ? w.cols : nullptr, strlen(w.cols));
            CHECK(bytes.size() == 11 * 28 + (cols ? 11 * 4 + 7 * 12 + 4 * 14 : 0)); // (without the columns: neither their length nor their bytes)
            words.close();
            CHECK(slurp(words.path) == bytes);
        }
}

int main(int argc, char **argv)
{
    if (argc > 1) scratch = argv[1];
    unsetenv("MALVA_GENO_HOST_ENUM");
    g_timers.on = false; // (MALVA_GENO_TIMERS in the environment: the timers' own lines are not this program's output)
    check_call_grown();
    check_call_times();
    check_one_sample();
    check_three_planes();
    check_host_fallback();
    check_cohort_priors();
    check_merged_rows();
    check_pipeline();
    check_site_words();
    std::cout << "call_worker_host_check: ok\n";
    return 0;
}
