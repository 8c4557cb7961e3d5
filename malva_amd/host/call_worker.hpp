// What a panel pass of `call` does between "a batch is closed" (host/panel_batch.hpp) and "its bytes are written": the batch's device calls, its
// text (host/call_text.hpp), and the pipeline that keeps as many batches in flight as there are devices.  Calls the ABI of include/malva_hip.h
// directly; tools/call_worker_host_check.cpp links it against an ABI of its own and drives all of it without a device (`make sanitize-host`).
#pragma once
#include <deque>
#include <future>
#include <iostream>
#include <memory>

#include "call_text.hpp"
#include "cohort_out.hpp"
#include "cohort_priors.hpp"
#include "device.hpp"
#include "options.hpp"

namespace malva {

// Device milliseconds (HIP events) and call counts of the batch calls behind the cohort's outputs.  A worker fills the one of its own batch
// (BatchText::times); whoever takes the batch adds it to the run's, so no two threads ever write one of them.
struct CallTimes {
    struct Kind {
        double ms[3] = {0, 0, 0};
        size_t calls[3] = {0, 0, 0};
        void add(const float *m, int n) // one call's n phases
        {
            for (int i = 0; i < n; ++i) ms[i] += m[i], ++calls[i];
        }
    };
    Kind format;   // --merged: mg_format_calls -- length pass, scan, write pass (calls[0] counts)
    Kind bcf;      // --merged-format bcf: mg_encode_calls_bcf, the same three
    Kind site;     // --site-tags: [0] mg_site_counts, [1] mg_format_site_info
    Kind pairs;    // --pairs: [0] mg_pack_dosage, [1] mg_pair_counts
    Kind sample;   // --sample-stats: mg_sample_counts
    Kind prior;    // --cohort-priors: mg_genotype_cohort
    Kind estimate; // --prior-groups: mg_estimate_priors
    Kind pl;       // --pl: mg_phred_likelihoods
    Kind geno;     // --site-stats: [0] mg_site_geno_counts, [1] mg_hwe_exact
    Kind ld;       // --ld: [0] mg_pack_site_dosage, [1] mg_ld_window
    Kind ibd;      // --ibd: [0] mg_pack_site_dosage (where --ld did not ask for the words already), [1] mg_ibd_step
    Kind grm;      // --grm: [0] mg_pack_site_dosage (where neither --ld nor --ibd asked), [1] mg_grm_step's weights + expansion, [2] its Gram kernel
    size_t gt_bytes = 0; // panel genotypes handed to mg_cover_blocks[_cohort]

    CallTimes &operator+=(const CallTimes &o)
    {
        Kind CallTimes::*const kinds[] = {&CallTimes::format, &CallTimes::bcf,   &CallTimes::site,    &CallTimes::pairs,
                                          &CallTimes::sample, &CallTimes::prior, &CallTimes::estimate, &CallTimes::pl,
                                          &CallTimes::geno,   &CallTimes::ld,   &CallTimes::ibd,
                                          &CallTimes::grm};
        for (auto k : kinds)
            for (int i = 0; i < 3; ++i) (this->*k).ms[i] += (o.*k).ms[i], (this->*k).calls[i] += (o.*k).calls[i];
        gt_bytes += o.gt_bytes;
        return *this;
    }
    // The sums of a cohort run under their labels in g_timers, in seconds: each with the timers on and its count non-zero.  Once per run, at its end.
    void add_to_timers() const
    {
        if (!g_timers.on) return;
        if (pairs.calls[1]) g_timers.add("pairs: pack and count kernels (device)", (pairs.ms[0] + pairs.ms[1]) / 1000.0);
        if (sample.calls[0]) g_timers.add("sample table: count kernel (device)", sample.ms[0] / 1000.0);
        if (geno.calls[0]) g_timers.add("site table: count and test kernels (device)", (geno.ms[0] + geno.ms[1]) / 1000.0);
        if (ld.calls[0]) g_timers.add("ld table: pack and window kernels (device)", (ld.ms[0] + ld.ms[1]) / 1000.0);
        if (ibd.calls[0] || ibd.calls[1]) g_timers.add("ibd table: pack and step kernels (device)", (ibd.ms[0] + ibd.ms[1]) / 1000.0);
        if (grm.calls[0] || grm.calls[1]) g_timers.add("grm: pack, weights, expand and gram kernels (device)", (grm.ms[0] + grm.ms[1] + grm.ms[2]) / 1000.0);
        if (prior.calls[0]) g_timers.add("cohort priors: kernel (device)", prior.ms[0] / 1000.0);
        if (estimate.calls[0]) g_timers.add("cohort priors: estimate kernel (device)", estimate.ms[0] / 1000.0);
        if (pl.calls[0]) g_timers.add("merged: likelihood kernel (device)", pl.ms[0] / 1000.0);
        if (bcf.calls[0]) g_timers.add("merged: encode kernels (device)", (bcf.ms[0] + bcf.ms[1] + bcf.ms[2]) / 1000.0);
        if (format.calls[0]) g_timers.add("merged: format kernels (device)", (format.ms[0] + format.ms[1] + format.ms[2]) / 1000.0);
    }
    // The lines of stderr behind a cohort run, under the same conditions; it changes nothing.  (mg_site_counts is reported beside the encoder for BCF
    // and beside mg_format_site_info for text; the pairs count pack and count apart.)
    std::string report() const
    {
        if (!g_timers.on) return std::string();
        std::string out;
        char line[256];
        if (pairs.calls[1]) {
            snprintf(line, sizeof line, "[malva-geno] pairs: %zu mg_pack_dosage, %zu mg_pair_counts, device ms per call: pack %.3f count %.3f\n", pairs.calls[0], pairs.calls[1],
                     pairs.calls[0] ? pairs.ms[0] / pairs.calls[0] : 0.0, pairs.ms[1] / pairs.calls[1]);
            out += line;
        }
        if (sample.calls[0]) {
            snprintf(line, sizeof line, "[malva-geno] sample-stats: %zu mg_sample_counts, device ms per call: count %.3f\n", sample.calls[0], sample.ms[0] / sample.calls[0]);
            out += line;
        }
        if (geno.calls[0]) {
            snprintf(line, sizeof line, "[malva-geno] site-stats: %zu mg_site_geno_counts, %zu mg_hwe_exact, device ms per call: count %.3f test %.3f\n", geno.calls[0],
                     geno.calls[1], geno.ms[0] / geno.calls[0], geno.calls[1] ? geno.ms[1] / geno.calls[1] : 0.0);
            out += line;
        }
        if (ld.calls[0]) {
            snprintf(line, sizeof line, "[malva-geno] ld: %zu mg_pack_site_dosage, %zu mg_ld_window, device ms per call: pack %.3f window %.3f\n", ld.calls[0], ld.calls[1],
                     ld.ms[0] / ld.calls[0], ld.calls[1] ? ld.ms[1] / ld.calls[1] : 0.0);
            out += line;
        }
        if (ibd.calls[0] || ibd.calls[1]) {
            snprintf(line, sizeof line, "[malva-geno] ibd: %zu mg_pack_site_dosage, %zu mg_ibd_step, device ms per call: pack %.3f step %.3f\n", ibd.calls[0], ibd.calls[1],
                     ibd.calls[0] ? ibd.ms[0] / ibd.calls[0] : 0.0, ibd.calls[1] ? ibd.ms[1] / ibd.calls[1] : 0.0);
            out += line;
        }
        if (grm.calls[0] || grm.calls[1]) {
            snprintf(line, sizeof line, "[malva-geno] grm: %zu mg_pack_site_dosage, %zu mg_grm_step, device ms per call: pack %.3f weights+expand %.3f gram %.3f\n", grm.calls[0],
                     grm.calls[1], grm.calls[0] ? grm.ms[0] / grm.calls[0] : 0.0, grm.calls[1] ? grm.ms[1] / grm.calls[1] : 0.0, grm.calls[1] ? grm.ms[2] / grm.calls[1] : 0.0);
            out += line;
        }
        if (prior.calls[0]) {
            snprintf(line, sizeof line, "[malva-geno] cohort-priors: %zu mg_genotype_cohort, device ms per call: %.3f\n", prior.calls[0], prior.ms[0] / prior.calls[0]);
            out += line;
        }
        if (estimate.calls[0]) {
            snprintf(line, sizeof line, "[malva-geno] cohort-priors: %zu mg_estimate_priors, device ms per call: %.3f\n", estimate.calls[0], estimate.ms[0] / estimate.calls[0]);
            out += line;
        }
        if (pl.calls[0]) {
            snprintf(line, sizeof line, "[malva-geno] merged: %zu mg_phred_likelihoods, device ms per call: %.3f\n", pl.calls[0], pl.ms[0] / pl.calls[0]);
            out += line;
        }
        if (bcf.calls[0]) {
            snprintf(line, sizeof line, "[malva-geno] merged: %zu mg_encode_calls_bcf, device ms per call: length %.3f scan %.3f write %.3f\n", bcf.calls[0],
                     bcf.ms[0] / bcf.calls[0], bcf.ms[1] / bcf.calls[0], bcf.ms[2] / bcf.calls[0]);
            out += line;
            if (site.calls[0]) {
                snprintf(line, sizeof line, "[malva-geno] merged: %zu mg_site_counts, device ms per call: count %.3f\n", site.calls[0], site.ms[0] / site.calls[0]);
                out += line;
            }
        }
        if (format.calls[0]) {
            snprintf(line, sizeof line, "[malva-geno] merged: %zu mg_format_calls, device ms per call: length %.3f scan %.3f write %.3f\n", format.calls[0],
                     format.ms[0] / format.calls[0], format.ms[1] / format.calls[0], format.ms[2] / format.calls[0]);
            out += line;
            if (site.calls[0] && site.calls[1]) {
                snprintf(line, sizeof line, "[malva-geno] merged: %zu mg_site_counts, %zu mg_format_site_info, device ms per call: count %.3f info %.3f\n", site.calls[0],
                         site.calls[1], site.ms[0] / site.calls[0], site.ms[1] / site.calls[1]);
                out += line;
            }
        }
        return out;
    }
};

// --pairs: a group's pair table so far -- [planes][planes][9], summed batch by batch (mg_pair_counts, B = A) -- and, when the cohort runs
// as several groups, the file that receives the packed words of the group's batches for the pass over pairs of groups
struct PairsRun {
    std::vector<uint64_t> counts;
    PartFile *pack_out = nullptr;
};

// Where one pass over the panel leaves what it makes; a member that is not set: the pass does not make it.
struct PassOut {
    std::deque<PartFile> per_sample; // sample p's text goes to per_sample[p] (empty: no per-sample text); they go with this object
    // --merged: the group's block of the multi-sample VCF -- a record's sample columns come as text from the device (mg_format_calls), behind
    // the record's fixed columns when merged_fixed, else on their own (a later group's columns, pasted behind the first group's lines at the end)
    PartFile *merged = nullptr;
    bool merged_fixed = false;
    // --site-tags: the records' allele counts over the group's planes are made beside the columns (mg_site_counts); not set: the group is the
    // cohort and INFO is made from them at once (mg_format_site_info), else they go here (put_site_counts) for the paste pass to sum over the groups
    PartFile *site_counts = nullptr;
    // --pairs: every batch's cells are packed into dosage bit planes (mg_pack_dosage) while the batch is in hand and counted against themselves
    // into pairs->counts; pairs->pack_out, when set, receives per batch and stream -- the lone records', then the others' -- the words (put_pack_batch)
    PairsRun *pairs = nullptr;
    // --sample-stats: the group's [planes][MG_SAMPLE_SLOTS] sums; every batch's cells are added while the batch is in hand (mg_sample_counts, accumulate)
    // (this table and pairs->counts are summed by the device call itself, batch after batch: the cohort's passes run on one device)
    uint64_t *sample_table = nullptr;
    // --site-stats: the records' genotype counts over the group's planes are made while the batch is in hand (mg_site_geno_counts).  The group is the
    // cohort: the ALTs are tested at once (mg_hwe_exact) and the table's lines go here.  site_stats_stream: the counts go here instead (put_site_geno,
    // with the records' columns when site_stats_cols) for the pass behind the last group to sum (site_stats_groups)
    PartFile *site_stats = nullptr;
    bool site_stats_stream = false, site_stats_cols = false;
    size_t site_stats_samples = 0; // the cohort's size
    // --ld, --ibd, --grm: the records' words over the group's planes are made while the batch is in hand (mg_pack_site_dosage) and go here in output
    // order (put_site_words, with the records' columns when site_words_cols): one stream for the passes behind the last group (ld_table, ibd_table,
    // grm_table).  site_words_for: the first of the three options that is given -- its timer and its CallTimes::Kind take the pack calls
    PartFile *site_words = nullptr;
    bool site_words_cols = false;
    enum SiteWordsFor { LD, IBD, GRM } site_words_for = LD;
    // --prior-groups, a cohort in several groups (host/cohort_priors.hpp).  prior_cov: the coverage pass -- the batches' coverages go here
    // (put_cov_batch; the first group's with the records' offsets and panel priors), and the pass makes no calls and nothing else.
    // prior_in: the output pass -- the batches' coverages and the cohort's frequencies come from here instead of the counters, and the
    // cells are genotyped under them by mg_genotype_cohort(iters = 0)
    PartFile *prior_cov = nullptr;
    bool prior_cov_panel = false;
    PriorGroupInput *prior_in = nullptr;
};
struct BatchText { // the text of one batch, as its worker hands it over
    std::vector<std::string> per_sample;
    std::string merged, site_counts, pack, priors, prior_cov, site_stats, site_words; // priors: the lines of --priors-out; prior_cov: the coverage pass's bytes
    CallTimes times; // of this batch's calls alone
};

// --merged-format bcf | ubcf: the merged file as BCF2 (host/bcf_out.hpp), a record's per-sample block encoded by mg_encode_calls_bcf
struct MergedFormat {
    bool bcf_out = false, bcf_bgzf = false;
    bool bcf_direct = false; // the cohort runs as one group: whole records leave the workers
    BcfHeader bcf_hdr;
    size_t bcf_samples = 0;  // the cohort's samples
    uint32_t n_fields(const Options &o) const { return (o.verbose ? 3 : 2) + (o.gp ? 1 : 0) + (o.pl ? 1 : 0); } // GT, GQ, COVS with -v, GP with --gp, PL with --pl
};

// --site-tags: the INFO strings of n records from their counts (mg_format_site_info), whoever holds the device
inline void site_info(Device &dev, size_t n, const uint32_t *ac, const uint32_t *ns, const uint32_t *var_allele_off, std::vector<char> &text, std::vector<uint64_t> &off,
                      CallTimes &times)
{
    off.resize(n + 1);
    text.resize(n * 40); // (a guess: the call says what it needs)
    dev.check(call_grown(text, [&](uint64_t *need) { return mg_format_site_info(dev.ctx, n, ac, ns, var_allele_off, text.data(), text.size(), off.data(), need); }),
              "mg_format_site_info");
    float ms[2] = {0, 0};
    dev.check(mg_site_stats(dev.ctx, ms), "mg_site_stats");
    times.site.ms[1] += ms[1];
    ++times.site.calls[1];
}

// One pass over the panel.  planes = 0: the one sample whose counters the context holds, text to to.per_sample[0] (stdout).  planes > 0:
// the context is in cohort mode; every batch goes up once and is covered for all planes, a record's fixed columns are made once and
// only the INFO and GT:GQ fields per sample.
// --cohort-priors: a batch's coverages are made as always; its frequencies are then re-estimated over all planes and every plane genotyped
// under them by ONE mg_genotype_cohort per batch kind, whose arrays everything below reads; priors_file, when open, gets a line per record.
// --prior-groups with a cohort in several groups: the pass runs twice per group -- to.prior_cov: up to the coverages, which it writes and
// nothing else; to.prior_in: coverages and the cohort's frequencies read back, the cells genotyped under them, everything below as always.
class PanelPass {
public:
    PanelPass(std::vector<Device> &devs, const Options &o, uint32_t planes, PassOut &to, size_t n_samples_kept, const MergedFormat &fmt, PriorsFile &priors_file,
              CallTimes &total)
        : devs(devs), o(o), planes(planes), P(planes ? planes : 1), to(to), n_samples((uint32_t)n_samples_kept), fmt(fmt), priors_file(priors_file), total(total)
    {
    }
    // One batch: device round trips, then the records' text.  Runs on a worker thread while the caller parses the next batch (the ABI has no
    // thread affinity); as many batches in flight as there are devices, and their text leaves in submission order.
    void submit(std::vector<Rec> &&recs, Batch &&iso, Batch &&gen)
    {
        drain(devs.size() - 1);
        if (to.prior_in) // (read here, on the one thread that hands the batches over: the streams keep the batches' order)
            for (Batch *b : {&iso, &gen})
                if (b->n()) to.prior_in->next(b == &gen, b->n(), b->var_allele_off.back(), b->cov, b->freq_out, b->n_inf);
        auto job = std::make_shared<Job>(Job{std::move(recs), std::move(iso), std::move(gen), jobs_started++ % devs.size()});
        in_flight.push_back(std::async(std::launch::async, [this, job]() { return process(*job); }));
    }
    void operator()(std::vector<Rec> &&recs, Batch &&iso, Batch &&gen) { submit(std::move(recs), std::move(iso), std::move(gen)); } // (what a BatchBuilder closes its batches with)
    void finish()
    {
        drain(0);
        if (to.prior_in) to.prior_in->done();
        for (PartFile &f : to.per_sample) fflush(f.f);
        if (to.merged) fflush(to.merged->f);
        if (to.site_counts) fflush(to.site_counts->f);
        if (to.site_stats) fflush(to.site_stats->f);
        if (to.site_words) fflush(to.site_words->f);
    }

private:
    struct Job {
        std::vector<Rec> recs;
        Batch iso, gen;
        size_t device = 0; // batches go round the devices: after the exchange every one of them holds the whole table's counters
    };
    struct MergedRows { // --merged: the sample columns of both batches, made where the genotypes were: [0] the lone records', [1] the others'
        std::vector<char> row_text[2], info_text[2];
        std::vector<uint64_t> row_off[2], info_off[2];
        std::vector<uint32_t> site_ac[2], site_ns[2];
    };
    struct SiteGeno { // --site-stats: the same two batches' counts, and (one group) the tests of their ALTs: record v's start at item_off[v]
        std::vector<uint32_t> n[2], het[2], hom[2];
        std::vector<size_t> item_off[2];
        std::vector<double> hwe[2], exc[2];
    };
    struct SiteWords { // --ld, --ibd, --grm: the same two batches' words, [3][records]
        std::vector<uint64_t> w[2];
    };

    std::vector<Device> &devs;
    const Options &o;
    const uint32_t planes;
    const size_t P;
    PassOut &to;
    const uint32_t n_samples; // the panel's kept samples
    const MergedFormat &fmt;
    PriorsFile &priors_file;
    CallTimes &total; // the run's: added to by drain alone
    const bool want_probs = o.verbose || o.gp; // the likelihood lists: GTS= of -v, GP of --merged --gp
    const bool tags = to.merged && o.site_tags;
    size_t jobs_started = 0;
    std::deque<std::future<BatchText>> in_flight; // (the last member: the workers are awaited before anything else of this object goes)

    void drain(size_t keep)
    {
        Timed t_drain("main: wait for worker + write");
        while (in_flight.size() > keep) {
            const BatchText text = in_flight.front().get(); // (or the batch's exception comes back here)
            in_flight.pop_front();
            total += text.times;
            for (size_t pl = 0; pl < to.per_sample.size(); ++pl) to.per_sample[pl].write(text.per_sample[pl], "cannot write the output");
            if (to.merged) to.merged->write(text.merged, "cannot write the merged output");
            if (to.site_counts) to.site_counts->write(text.site_counts, "cannot write the merged output's counts");
            if (to.pairs && to.pairs->pack_out) to.pairs->pack_out->write(text.pack, "cannot write the pair table's packed calls");
            priors_file.write(text.priors);
            if (to.prior_cov) to.prior_cov->write(text.prior_cov, "cannot write the coverages for the cohort's priors");
            if (to.site_stats) to.site_stats->write(text.site_stats, to.site_stats_stream ? "cannot write the per-record table's counts" : "cannot write the per-record table");
            if (to.site_words) to.site_words->write(text.site_words, "cannot write the records' site words");
        }
    }

    BatchText process(Job &job)
    {
        Batch &iso = job.iso, &gen = job.gen;
        Device &dev = devs[job.device];
        BatchText text;
        text.per_sample.resize(to.per_sample.size());
        MergedRows rows;
        SiteGeno geno;
        SiteWords words;
        {
            Timed t_dev("worker: device calls");
            std::lock_guard<std::mutex> device_lock(dev.mu); // (the parsing thread cuts blocks on device 0 meanwhile)
            if (iso.n()) lone_calls(dev, iso);
            if (iso.n() && o.priors.on && !to.prior_cov) cohort_priors(dev, iso, text.times); // (mg_call_isolated made the coverages; its calls are replaced)
            if (gen.n()) {
                size_results(gen);
                if (!to.prior_in) cover_blocks(dev, gen, text.times); // (the output pass of a cohort in several groups has the coverages from the group's file)
                if (to.prior_cov) {} // (the coverage pass makes no calls)
                else if (o.priors.on) cohort_priors(dev, gen, text.times);
                else plane_genotypes(dev, gen);
            }
            if (to.prior_cov) { // the coverage pass: the batches' coverages for the estimate pass, and nothing else
                for (int w = 0; w < 2; ++w) {
                    const Batch &b = w ? gen : iso;
                    if (b.n()) put_cov_batch(text.prior_cov, (uint64_t)w, b.n(), b.var_allele_off.data(), b.freq.data(), to.prior_cov_panel, P, b.cov.data());
                }
                return text;
            }
            if (to.merged && o.pl) phred_likelihoods(dev, job, text.times);
            if (to.merged) merged_rows(dev, job, rows, text.times);
            if (to.pairs) pair_table(dev, job, text);
            if (to.sample_table) sample_table(dev, job, text.times);
            if (to.site_stats) site_table(dev, job, geno, text.times);
            if (to.site_words) site_words(dev, job, words, text.times);
        } // the records' text needs no device
        records_text(job, rows, geno, words, text);
        return text;
    }

    // a batch's result arrays at their sizes: [plane][record], [plane][allele slot], [plane][genotype slot]
    void size_results(Batch &b) const
    {
        const size_t n = b.n(), na = b.var_allele_off.back(), ng = want_probs ? b.var_gt_off.back() : 0;
        b.cov.resize(P * na); b.g1.resize(P * n); b.g2.resize(P * n); b.gq.resize(P * n); b.status.resize(P * n);
        b.probs.resize(P * ng);
    }

    void lone_calls(Device &dev, Batch &iso)
    {
        const size_t n = iso.n(), na = iso.var_allele_off.back(), ng = want_probs ? iso.var_gt_off.back() : 0;
        size_results(iso);
        for (size_t pl = 0; pl < P && !to.prior_in; ++pl) { // (the fused lone-variant call reads the selected plane)
            if (planes) dev.check(mg_cohort_select(dev.ctx, (uint32_t)pl), "mg_cohort_select");
            dev.check(mg_call_isolated(dev.ctx, n, iso.pos.data(), iso.var_allele_off.data(), iso.allele_off.data(), iso.pool.data(), iso.pool.size(),
                                       iso.freq.data(), iso.present.data(), iso.flags.data(), o.error_rate, (int)o.max_coverage, o.haploid, iso.cov.data() + pl * na,
                                       iso.g1.data() + pl * n, iso.g2.data() + pl * n, iso.gq.data() + pl * n, iso.status.data() + pl * n,
                                       want_probs ? iso.probs.data() + pl * ng : nullptr, want_probs ? iso.var_gt_off.data() : nullptr),
                      "mg_call_isolated");
        }
    }

    // the general blocks' coverages: one call for the whole batch, in the form the panel's genotypes and the pass take; then the blocks it handed back
    void cover_blocks(Device &dev, Batch &gen, CallTimes &times)
    {
        const size_t n = gen.n();
        // panel genotypes of the batch as one [variant][sample] matrix of a1 | a2 << 7 | phased << 14
        std::vector<uint8_t> overflow(n, 0);
        bool device_ok = o.k <= MG_MAX_PACKED_K && !getenv("MALVA_GENO_HOST_ENUM"); // the variable forces the host enumerator (tests)
        if (gen.wide_alleles) device_ok = false;
        PanelGenotypes pg;
        if (gen.dense_gt) pg.gt = std::move(gen.gt_dense);
        else pg = pack_genotypes(gen.vars, n, n_samples, o.haploid); // (every record of such a batch is kept)
        times.gt_bytes += pg.bytes();
        const mg_blocks_host x = gen.view(pg, n_samples);
        if (device_ok && planes) // the batch goes up once and is covered for every plane (cov: [planes][na])
            dev.check(mg_cover_blocks_cohort(dev.ctx, &x, o.haploid, gen.cov.data(), overflow.data()), "mg_cover_blocks_cohort");
        else if (device_ok)
            dev.check(mg_cover_blocks(dev.ctx, &x, o.haploid, gen.cov.data(), overflow.data()), "mg_cover_blocks"); // extract_kmers + set_coverages, main.cpp:556-557
        else
            std::fill(overflow.begin(), overflow.end(), 1);
        host_fallback(dev, gen, overflow);
    }

    // blocks the device handed back (a capacity was exceeded, or a window was clipped by a contig end):
    // host enumerator + mg_lookup_cover for exactly those blocks
    void host_fallback(Device &dev, Batch &gen, const std::vector<uint8_t> &overflow)
    {
        const size_t na = gen.var_allele_off.back();
        size_t n_fallback = 0;
        for (size_t b = 0; b < gen.n_blocks(); ++b) {
            bool redo = false;
            for (uint32_t v = gen.blk_var_off[b]; v < gen.blk_var_off[b + 1]; ++v) redo = redo || overflow[v];
            if (!redo) continue;
            ++n_fallback;
            Block blk((int)o.k); // (rebuilt from the batch's records: nothing reads them after this)
            for (uint32_t v = gen.blk_var_off[b]; v < gen.blk_var_off[b + 1]; ++v) {
                if (gen.var_slot[v] < 0) throw std::runtime_error("internal: the device handed back a record tier 1 should have taken");
                blk.add(std::move(gen.vars[(size_t)gen.var_slot[v]]));
            }
            genotypes_from_entries(blk);
            const SignatureRows s = signature_rows(blk, blk.extract(*gen.block_ref[b], o.haploid));
            const size_t slot0 = gen.var_allele_off[gen.blk_var_off[b]];
            for (size_t pl = 0; pl < P; ++pl) { // (enumerated once; the lookups read the selected plane)
                if (planes) dev.check(mg_cohort_select(dev.ctx, (uint32_t)pl), "mg_cohort_select");
                dev.check(mg_lookup_cover(dev.ctx, s.rows.data.data(), STRIDE, s.rows.n, s.is_ref.data(), s.sig_off.data(), s.sig_off.size() - 1, s.al_off.data(),
                                          s.al_off.size() - 1, gen.cov.data() + pl * na + slot0),
                          "mg_lookup_cover");
            }
        }
        if (n_fallback) std::cerr << "[malva-geno] " << n_fallback << " block(s) enumerated on the host" << std::endl;
    }

    void plane_genotypes(Device &dev, Batch &gen)
    {
        const size_t n = gen.n(), na = gen.var_allele_off.back(), ng = want_probs ? gen.var_gt_off.back() : 0;
        for (size_t pl = 0; pl < P; ++pl)
            dev.check(mg_genotype(dev.ctx, gen.cov.data() + pl * na, gen.freq.data(), gen.var_allele_off.data(), n, o.error_rate, (int)o.max_coverage, o.haploid,
                                  gen.g1.data() + pl * n, gen.g2.data() + pl * n, gen.gq.data() + pl * n, gen.status.data() + pl * n,
                                  want_probs ? gen.probs.data() + pl * ng : nullptr, want_probs ? gen.var_gt_off.data() : nullptr),
                      "mg_genotype"); // vb.genotype + the GT/GQ part of output_variants, main.cpp:558-559
    }

    // the batch's priors from all of its planes, and the planes' calls under them
    void cohort_priors(Device &dev, Batch &b, CallTimes &times)
    {
        Timed t_prior("worker: cohort priors (mg_genotype_cohort)");
        const bool prior_in = to.prior_in != nullptr;
        const size_t n = b.n(), ng = want_probs ? b.var_gt_off.back() : 0;
        b.freq_out.resize(b.freq.size());
        b.n_inf.resize(n);
        b.probs.resize(P * ng);
        // the output pass of a cohort in several groups: freq_out and n_inf hold the cohort's estimate; the cells under it, nothing re-estimated
        const std::vector<float> f_t = prior_in ? b.freq_out : std::vector<float>();
        std::vector<uint32_t> no_n(prior_in ? n : 0);
        dev.check(mg_genotype_cohort(dev.ctx, n, (uint32_t)P, b.cov.data(), prior_in ? f_t.data() : b.freq.data(), b.var_allele_off.data(), o.error_rate,
                                     (int)o.max_coverage, o.haploid, prior_in ? 0 : o.priors.iters, o.priors.weight, b.freq_out.data(),
                                     prior_in ? no_n.data() : b.n_inf.data(), b.g1.data(), b.g2.data(), b.gq.data(), b.status.data(),
                                     want_probs ? b.probs.data() : nullptr, want_probs ? b.var_gt_off.data() : nullptr),
                  "mg_genotype_cohort");
        float ms = 0;
        dev.check(mg_cohort_prior_stats(dev.ctx, &ms), "mg_cohort_prior_stats");
        times.prior.add(&ms, 1);
    }

    // --pl: the Phred-scaled likelihoods of a batch's cells from its coverages, whoever made those (mg_call_isolated, the record loop, the
    // group's scratch file): one call over all planes per batch kind
    void phred_likelihoods(Device &dev, Job &job, CallTimes &times)
    {
        Timed t_pl("worker: likelihoods (mg_phred_likelihoods)");
        for (Batch *b : {&job.iso, &job.gen}) {
            if (!b->n()) continue;
            b->pl.resize(P * (size_t)b->var_gt_off.back());
            dev.check(mg_phred_likelihoods(dev.ctx, b->n(), (uint32_t)P, b->cov.data(), b->var_allele_off.data(), b->var_gt_off.data(), o.error_rate, (int)o.max_coverage,
                                           o.haploid, o.pl_cap, b->pl.data()),
                      "mg_phred_likelihoods");
            float ms = 0;
            dev.check(mg_pl_stats(dev.ctx, &ms), "mg_pl_stats");
            times.pl.add(&ms, 1);
        }
    }

    // one batch's sample columns: text or BCF, with or without GP, PL and the GQ mask
    int format_rows(Device &dev, Batch &b, std::vector<char> &text, std::vector<uint64_t> &off, uint64_t *need)
    {
        const bool lists = o.gp || o.pl; // (a field per genotype: the records' alleles and genotype slots are needed)
        mg_cells x{};
        x.n_vars = b.n(), x.n_planes = (uint32_t)P, x.haploid = o.haploid;
        x.gt1 = b.g1.data(), x.gt2 = b.g2.data(), x.gq = b.gq.data();
        x.use_mask = o.use_min_gq, x.min_gq = o.min_gq;
        if (o.verbose) x.cov = b.cov.data();
        if (o.verbose || lists) x.var_allele_off = b.var_allele_off.data();
        if (lists) x.var_gt_off = b.var_gt_off.data();
        if (o.gp) x.probs = b.probs.data(), x.status = b.status.data();
        if (o.pl) x.pl = b.pl.data();
        x.fields = (o.gp ? MG_CELLS_GP : 0) | (o.pl ? MG_CELLS_PL : 0);
        if (!fmt.bcf_out) return mg_format_calls(dev.ctx, &x, text.data(), text.size(), off.data(), need);
        const BcfHeader &hdr = fmt.bcf_hdr;
        const mg_bcf_keys keys{hdr.key("GT"), hdr.key("GQ"), o.verbose ? hdr.key("COVS") : 0, o.gp ? hdr.key("GP") : 0, o.pl ? hdr.key("PL") : 0};
        return mg_encode_calls_bcf(dev.ctx, &x, &keys, (uint8_t *)text.data(), text.size(), off.data(), need);
    }

    void merged_rows(Device &dev, Job &job, MergedRows &rows, CallTimes &times)
    {
        Timed t_fmt(fmt.bcf_out ? "worker: merged rows (mg_encode_calls_bcf)" : "worker: merged rows (mg_format_calls)");
        for (int w = 0; w < 2; ++w) {
            Batch &b = w ? job.gen : job.iso;
            const size_t bn = b.n();
            if (!bn) continue;
            rows.row_off[w].resize(bn + 1);
            rows.row_text[w].resize(bn * (P * (o.haploid ? 8 : 10) + 1) + (o.verbose ? 4 * P * (size_t)b.var_allele_off.back() : 0) +
                                    (o.gp ? P * (bn + (fmt.bcf_out ? 4 : 9) * (size_t)b.var_gt_off.back()) : 0) +
                                    (o.pl ? P * (bn + (fmt.bcf_out ? 2 : 4) * (size_t)b.var_gt_off.back()) : 0)); // (a guess: the call says what it needs)
            dev.check(call_grown(rows.row_text[w], [&](uint64_t *need) { return format_rows(dev, b, rows.row_text[w], rows.row_off[w], need); }),
                      fmt.bcf_out ? "mg_encode_calls_bcf" : "mg_format_calls");
            float ms[3] = {0, 0, 0};
            if (fmt.bcf_out) {
                dev.check(mg_bcf_stats(dev.ctx, ms), "mg_bcf_stats");
                for (int i = 0; i < 3; ++i) times.bcf.ms[i] += ms[i];
                ++times.bcf.calls[0];
            } else {
                dev.check(mg_format_stats(dev.ctx, ms), "mg_format_stats");
                for (int i = 0; i < 3; ++i) times.format.ms[i] += ms[i];
                ++times.format.calls[0];
            }
            if (!tags) continue;
            rows.site_ac[w].resize(b.var_allele_off.back());
            rows.site_ns[w].resize(bn);
            dev.check(mg_site_counts(dev.ctx, bn, (uint32_t)P, o.haploid, b.g1.data(), b.g2.data(), b.gq.data(), o.use_min_gq, o.min_gq, b.var_allele_off.data(), 0,
                                     rows.site_ac[w].data(), rows.site_ns[w].data()),
                      "mg_site_counts");
            dev.check(mg_site_stats(dev.ctx, ms), "mg_site_stats");
            times.site.add(ms, 1);
            if (!to.site_counts && !fmt.bcf_out) site_info(dev, bn, rows.site_ac[w].data(), rows.site_ns[w].data(), b.var_allele_off.data(), rows.info_text[w], rows.info_off[w], times);
        }
    }

    void pair_table(Device &dev, Job &job, BatchText &text)
    {
        Timed t_pairs("worker: pair table (mg_pack_dosage, mg_pair_counts)");
        std::vector<uint64_t> words;
        for (int w = 0; w < 2; ++w) {
            Batch &b = w ? job.gen : job.iso;
            const size_t bn = b.n(), W = (bn + 63) / 64;
            if (!bn) continue;
            words.resize(P * 3 * W);
            dev.check(mg_pack_dosage(dev.ctx, bn, (uint32_t)P, o.haploid, b.g1.data(), b.g2.data(), b.gq.data(), o.use_min_gq, o.min_gq, b.var_allele_off.data(),
                                     words.data()),
                      "mg_pack_dosage");
            dev.check(mg_pair_counts(dev.ctx, W, words.data(), (uint32_t)P, nullptr, (uint32_t)P, 1, to.pairs->counts.data()), "mg_pair_counts");
            float ms[2] = {0, 0};
            dev.check(mg_pairs_stats(dev.ctx, ms), "mg_pairs_stats");
            text.times.pairs.add(ms, 2);
            if (to.pairs->pack_out) put_pack_batch(text.pack, (uint64_t)w, bn, words);
        }
    }

    void sample_table(Device &dev, Job &job, CallTimes &times)
    {
        Timed t_sample("worker: sample table (mg_sample_counts)");
        for (int w = 0; w < 2; ++w) {
            Batch &b = w ? job.gen : job.iso;
            const size_t bn = b.n();
            if (!bn) continue;
            dev.check(mg_sample_counts(dev.ctx, bn, (uint32_t)P, o.haploid, b.g1.data(), b.g2.data(), b.gq.data(), o.use_min_gq, o.min_gq, b.status.data(), b.cov.data(),
                                       b.var_allele_off.data(), b.allele_class.data(), 1, to.sample_table),
                      "mg_sample_counts");
            float ms = 0;
            dev.check(mg_sample_stats(dev.ctx, &ms), "mg_sample_stats");
            times.sample.add(&ms, 1);
        }
    }

    void site_table(Device &dev, Job &job, SiteGeno &g, CallTimes &times)
    {
        Timed t_site("worker: site table (mg_site_geno_counts, mg_hwe_exact)");
        std::vector<uint32_t> item_n, item_het, item_hom;
        for (int w = 0; w < 2; ++w) {
            Batch &b = w ? job.gen : job.iso;
            const size_t bn = b.n();
            if (!bn) continue;
            g.n[w].resize(bn);
            g.het[w].resize(b.var_allele_off.back());
            g.hom[w].resize(b.var_allele_off.back());
            dev.check(mg_site_geno_counts(dev.ctx, bn, (uint32_t)P, o.haploid, b.g1.data(), b.g2.data(), b.gq.data(), o.use_min_gq, o.min_gq, b.var_allele_off.data(), 0,
                                          g.n[w].data(), g.het[w].data(), g.hom[w].data()),
                      "mg_site_geno_counts");
            float ms[2] = {0, 0};
            dev.check(mg_hwe_stats(dev.ctx, ms), "mg_hwe_stats");
            times.geno.add(ms, 1);
            if (to.site_stats_stream || o.haploid) continue; // (the pass behind the last group tests the sums; a haploid table has no test)
            item_n.clear(), item_het.clear(), item_hom.clear();
            g.item_off[w].resize(bn);
            for (size_t v = 0; v < bn; ++v) {
                g.item_off[w][v] = item_n.size();
                site_stats_items(b.var_allele_off[v + 1] - b.var_allele_off[v], g.n[w][v], &g.het[w][b.var_allele_off[v]], &g.hom[w][b.var_allele_off[v]], item_n, item_het,
                                 item_hom);
            }
            g.hwe[w].resize(item_n.size());
            g.exc[w].resize(item_n.size());
            if (item_n.empty()) continue;
            dev.check(mg_hwe_exact(dev.ctx, item_n.size(), item_n.data(), item_het.data(), item_hom.data(), g.hwe[w].data(), g.exc[w].data()), "mg_hwe_exact");
            dev.check(mg_hwe_stats(dev.ctx, ms), "mg_hwe_stats");
            times.geno.ms[1] += ms[1];
            ++times.geno.calls[1];
        }
    }

    void site_words(Device &dev, Job &job, SiteWords &sw, CallTimes &times)
    {
        const PassOut::SiteWordsFor asked = to.site_words_for;
        Timed t_words(asked == PassOut::LD ? "worker: ld words (mg_pack_site_dosage)" : asked == PassOut::IBD ? "worker: ibd words (mg_pack_site_dosage)" : "worker: grm words (mg_pack_site_dosage)");
        for (int w = 0; w < 2; ++w) {
            Batch &b = w ? job.gen : job.iso;
            const size_t bn = b.n();
            if (!bn) continue;
            sw.w[w].resize(3 * bn);
            dev.check(mg_pack_site_dosage(dev.ctx, bn, (uint32_t)P, o.haploid, b.g1.data(), b.g2.data(), b.gq.data(), o.use_min_gq, o.min_gq, b.var_allele_off.data(),
                                          sw.w[w].data()),
                      "mg_pack_site_dosage");
            float ms[2] = {0, 0};
            dev.check(mg_ld_stats(dev.ctx, ms), "mg_ld_stats");
            (asked == PassOut::LD ? times.ld : asked == PassOut::IBD ? times.ibd : times.grm).add(ms, 1);
        }
    }

    void records_text(const Job &job, const MergedRows &rows, const SiteGeno &geno, const SiteWords &words, BatchText &text)
    {
        Timed t_text("worker: records' text");
        const Batch &iso = job.iso, &gen = job.gen;
        for (const Rec &r : job.recs) {
            const Batch &b = r.isolated ? iso : gen;
            const int w = r.isolated ? 0 : 1;
            if (priors_file.f) priors_row(text.priors, r.prefix, r.n_alleles, b.freq.data() + r.allele0, b.freq_out.data() + r.allele0, b.n_inf[r.slot]);
            if (tags && to.site_counts) put_site_counts(text.site_counts, r.n_alleles, rows.site_ns[w][r.slot], rows.site_ac[w].data() + r.allele0);
            if (to.site_words) {
                const std::vector<uint64_t> &sw = words.w[w];
                const size_t bn = sw.size() / 3;
                put_site_words(text.site_words, sw[r.slot], sw[bn + r.slot], sw[2 * bn + r.slot], r.n_alleles, to.site_words_cols ? r.prefix.data() : nullptr,
                               site_stats_cols(r.prefix));
            }
            if (!to.site_stats) continue;
            const uint32_t *het = geno.het[w].data() + r.allele0, *hom = geno.hom[w].data() + r.allele0;
            const size_t cols = site_stats_cols(r.prefix);
            if (to.site_stats_stream) put_site_geno(text.site_stats, r.n_alleles, geno.n[w][r.slot], het, hom, to.site_stats_cols ? r.prefix.data() : nullptr, cols);
            else {
                const size_t item = o.haploid ? 0 : geno.item_off[w][r.slot];
                site_stats_row(text.site_stats, r.prefix.data(), cols, to.site_stats_samples, o.haploid, r.n_alleles, geno.n[w][r.slot], het, hom, geno.hwe[w].data() + item,
                               geno.exc[w].data() + item);
            }
        }
        if (to.merged && fmt.bcf_out)
            merged_bcf_records(text.merged, job.recs, rows.row_text, rows.row_off, rows.site_ac, rows.site_ns, fmt.bcf_hdr, fmt.n_fields(o), (uint32_t)P, to.merged_fixed,
                               fmt.bcf_direct, tags, fmt.bcf_bgzf);
        else if (to.merged) // (INFO stays '.' in a block: the paste pass puts it in)
            merged_text_lines(text.merged, job.recs, rows.row_text, rows.row_off, rows.info_text, rows.info_off, o.verbose, o.gp, to.merged_fixed, tags && !to.site_counts, o.pl);
        if (!to.per_sample.empty()) per_sample_lines(text.per_sample, job.recs, iso, gen, P, o.haploid, o.verbose, o.max_coverage);
    }
};

} // namespace malva
