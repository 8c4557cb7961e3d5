// malva-geno index|call -- host driver of the MI355X-native hot path.
//
// Keeps the reference's command line (argument_parser.hpp:51-159), control flow
// (index_main main.cpp:251-419, call_main :421-594) and VCF output, and hands
// every k-mer store operation, both scans, coverage and likelihoods to
// libmalva_hip.so through include/malva_hip.h.  There is no CPU implementation of
// those in this program: without a GPU it stops at mg_create.
#include <fcntl.h>
#include <functional>
#include <future>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <iostream>
#include <mutex>
#include <sstream>
#include <thread>

#include "block.hpp"
#include "index_file.hpp"
#include "kmc_db.hpp"
#include "reads.hpp"
#include "cohort.hpp"
#include "bcf_out.hpp"
#include "cohort_priors.hpp"
#include "options.hpp"
#include "usage.hpp"
#include "cohort_out.hpp"
#include "call_worker.hpp"
#include "pca.hpp"

using namespace malva;

namespace {

// pelapsed(), main.cpp:93-115
auto t_start = std::chrono::steady_clock::now();
auto t_last = t_start;
void pelapsed(const std::string &s, bool rollback = false)
{
    const auto now = std::chrono::steady_clock::now();
    rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    char buf[512];
    snprintf(buf, sizeof buf, "[malva-geno/%s] Execution Time %.4gs\n[malva-geno/%s] Time elapsed %.4gs\n[malva-geno/%s] Used CPU-time elapsed %.4gs\n"
                              "[malva-geno/%s] Maximum memory used %ldMb\n",
             s.c_str(), std::chrono::duration<double>(now - t_last).count(), s.c_str(), std::chrono::duration<double>(now - t_start).count(), s.c_str(),
             ru.ru_utime.tv_sec + ru.ru_utime.tv_usec * 1e-6, s.c_str(), ru.ru_maxrss / 1024);
    std::cerr << buf << (rollback ? "\r" : "\n");
    t_last = now;
}

// main.cpp:407 / :456: <vcf>.c<ref_k>.k<k>.malvax + ".zst" (the reference's container) or ".hipz" (this build's compact one)
std::string index_path(const Options &o, const char *suffix)
{
    return o.vcf_path + ".c" + std::to_string(o.ref_k) + ".k" + std::to_string(o.k) + ".malvax" + suffix;
}

// ---- genotypes the reader left to the device (VcfReader::defer_genotypes) ---------------------------------------------------
// A panel of a thousand samples or more has its sample columns decoded on the device (MALVA_GENO_GT_DEVICE=0 / 1 forces either way;
// the reader defers only where it can: a text file read through the pool).
inline bool device_gt_wanted(const VcfReader &vcf)
{
    if (const char *e = getenv("MALVA_GENO_GT_DEVICE")) return atoi(e) != 0;
    return vcf.keep.size() >= 1024;
}
// The records of one cut batch, block of text by block of text: mg_decode_gt_text over the spans, the entries back into the records.
struct GtDecodeCount {
    size_t records = 0, calls = 0, on_host = 0; // records decoded on the device, in so many calls; of them, handed to the host decoder after all
};
inline void decode_deferred(std::vector<Variant> &kept, Device &dev, VcfReader &vcf, const Options &o, GtDecodeCount &count)
{
    std::vector<uint64_t> off, mask;
    std::vector<uint32_t> len, sp_off, mx, ss;
    std::vector<int32_t> gi;
    std::vector<uint16_t> sg;
    std::vector<uint8_t> keep_cols(vcf.samples.size(), 0);
    for (int i : vcf.keep) keep_cols[(size_t)i] = 1;
    for (size_t a = 0; a < kept.size();) {
        if (!kept[a].gt_deferred) {
            ++a;
            continue;
        }
        size_t b = a;
        while (b < kept.size() && kept[b].gt_deferred && kept[b].gt_text == kept[a].gt_text) ++b;
        const size_t n = b - a;
        off.resize(n); len.resize(n); gi.resize(n); sp_off.resize(n + 1); mask.resize(n); mx.resize(n);
        for (size_t r = 0; r < n; ++r) {
            off[r] = kept[a + r].gt_off;
            len[r] = kept[a + r].gt_len;
            gi[r] = kept[a + r].gt_index;
        }
        uint16_t dflt = 0;
        uint64_t n_entries = 0;
        {
            Timed t("main: mg_decode_gt_text (+ lock)");
            std::lock_guard<std::mutex> lk(dev.mu);
            const std::string &text = *kept[a].gt_text;
            dev.check(mg_decode_gt_text(dev.ctx, text.data(), text.size(), n, off.data(), len.data(), gi.data(), (uint32_t)keep_cols.size(), keep_cols.data(), o.haploid,
                                        &dflt, sp_off.data(), mask.data(), mx.data(), &n_entries),
                      "mg_decode_gt_text");
            ss.resize(n_entries);
            sg.resize(n_entries);
            dev.check(mg_decode_gt_entries(dev.ctx, ss.data(), sg.data()), "mg_decode_gt_entries");
        }
        count.records += n;
        ++count.calls;
        for (size_t r = 0; r < n; ++r) {
            Variant &v = kept[a + r];
            v.sp_default = dflt;
            v.raw_mask = mask[r];
            v.max_allele = mx[r];
            if (mx[r] > 127) { // an allele number the 7-bit words cannot hold: this record is decoded here after all
                vcf.genotypes_on_host(v);
                ++count.on_host;
                continue;
            }
            v.sp_sample.assign(ss.begin() + sp_off[r], ss.begin() + sp_off[r + 1]);
            v.sp_gt.assign(sg.begin() + sp_off[r], sg.begin() + sp_off[r + 1]);
            v.gt_text.reset(); // (the block of text goes when its last record has let go)
        }
        a = b;
    }
}

// The record loop shared by index_main (main.cpp:309-370) and call_main (:522-579).  on_block(block, reference
// of `last_seq_name`) is called for every closed block.  Keeps the reference's control flow, including that
// last_seq_name is refreshed only when a block is flushed.
// `cutter` (optional): the device that makes the cuts (mg_cut_blocks) -- the kept records are then collected a batch at a
// time and the loop below is replayed over the device's block offsets; without it (dump-kmers, MALVA_GENO_HOST_CUT=1) the
// cuts are made record by record on the host.  Same blocks either way (tests/test_gpu_cli.py runs both).
template <class F> size_t for_each_block(VcfReader &vcf, const Options &o, const Reference &refs, bool for_index, std::vector<std::string> *used, F on_block,
                                         Device *cutter = nullptr)
{
    static const std::string empty;
    std::string ref_name;            // (a panel names a few dozen sequences over millions of records: the last answer is nearly always the next one)
    const std::string *ref_seq = nullptr;
    auto ref_of = [&](const std::string &name) -> const std::string & {
        if (!ref_seq || name != ref_name) {
            auto it = refs.seqs.find(name);
            ref_seq = it == refs.seqs.end() ? &empty : &it->second;
            ref_name = name;
        }
        return *ref_seq;
    };
    if (cutter && !getenv("MALVA_GENO_HOST_CUT")) {
        // records per cut batch; MALVA_GENO_CUT_BATCH exists so tests can put a batch seam inside every block
        const size_t batch_max = getenv("MALVA_GENO_CUT_BATCH") ? (size_t)std::max(1L, atol(getenv("MALVA_GENO_CUT_BATCH"))) : 100000;
        Block vb((int)o.k);          // the open block: the records since the last cut
        std::string block_name;      // `last_seq_name` of the reference loop: the name the open block will be flushed under
        uint32_t last_cid = 0;       // contig id the open block's last record presents to the next one
        std::map<std::string, uint32_t> ids;
        auto id_of = [&](const std::string &name) { return ids.emplace(name, (uint32_t)ids.size()).first->second; };
        std::vector<Variant> kept;
        std::vector<int32_t> pos;
        std::vector<uint32_t> ref_size, min_size, cid, off;
        size_t i = 0, cells = 0, n_cut_blocks = 0, n_batches = 0;
        bool more = true, seen_kept = false;
        GtDecodeCount gt_count;
        Variant v;
        while (more) {
            kept.clear();
            cells = 0;
            Timed *t_parse = new Timed("main: vcf.next");
            while (kept.size() < batch_max && cells < (64u << 20) && (more = vcf.next(v, o.freq_key, o.uniform))) {
                ++i;
                if (i % 5000 == 0) pelapsed("Processed " + std::to_string(i) + " variants", true);
                if (block_name.empty()) { // the file's first record names the first block, kept or not (main.cpp:319-323)
                    block_name = v.seq_name;
                    if (used) used->push_back(block_name);
                }
                if (for_index ? (!v.has_alts || !v.is_present) : !v.has_alts) continue;
                cells += v.n_genotypes();
                kept.push_back(std::move(v));
            }
            delete t_parse;
            if (kept.empty()) continue;
            decode_deferred(kept, *cutter, vcf, o, gt_count);
            const bool carry = !vb.empty();
            const size_t n = kept.size() + (carry ? 1 : 0);
            pos.resize(n); ref_size.resize(n); min_size.resize(n); cid.resize(n); off.resize(n + 1);
            if (carry) {
                const Variant &c = vb.vars.back();
                pos[0] = c.ref_pos; ref_size[0] = (uint32_t)c.ref_size; min_size[0] = (uint32_t)c.min_size; cid[0] = last_cid;
            }
            for (size_t j = 0; j < kept.size(); ++j) {
                const Variant &r = kept[j];
                const size_t q = j + (carry ? 1 : 0);
                pos[q] = r.ref_pos; ref_size[q] = (uint32_t)r.ref_size; min_size[q] = (uint32_t)r.min_size;
                // the very first kept record is added to an empty block unseen; what the NEXT record compares its name with
                // is `last_seq_name`, still the file's first name then
                cid[q] = seen_kept ? id_of(r.seq_name) : id_of(block_name);
                seen_kept = true;
            }
            size_t nb = 0;
            {
                Timed t_cut("main: mg_cut_blocks (+ lock)");
                std::lock_guard<std::mutex> lk(cutter->mu);
                cutter->check(mg_cut_blocks(cutter->ctx, n, pos.data(), ref_size.data(), min_size.data(), cid.data(), off.data(), &nb), "mg_cut_blocks");
            }
            last_cid = cid[n - 1];
            ++n_batches;
            size_t b = 0; // off[b] = next block start at or after the current element
            Timed t_blocks("main: blocks -> batches");
            for (size_t q = carry ? 1 : 0; q < n; ++q) {
                while (b < nb && off[b] < q) ++b;
                const bool cut = b < nb && off[b] == q;
                Variant &r = kept[q - (carry ? 1 : 0)];
                if (cut && !vb.empty()) {
                    on_block(vb, block_name, ref_of(block_name));
                    ++n_cut_blocks;
                    vb.clear();
                    if (block_name != r.seq_name) {
                        block_name = r.seq_name;
                        if (used) used->push_back(block_name);
                    }
                }
                vb.add(std::move(r));
            }
        }
        if (!vb.empty()) {
            on_block(vb, block_name, ref_of(block_name));
            ++n_cut_blocks;
            vb.clear();
        }
        std::cerr << "[malva-geno] " << n_cut_blocks << " block(s) cut on the device in " << n_batches << " batch(es)" << std::endl;
        if (gt_count.calls)
            std::cerr << "[malva-geno] sample columns of " << gt_count.records << " record(s) decoded on the device in " << gt_count.calls << " call(s), "
                      << gt_count.on_host << " of them handed to the host decoder" << std::endl;
        return i;
    }
    Block vb((int)o.k);
    std::string last_seq_name;
    Variant v;
    size_t i = 0;
    while (vcf.next(v, o.freq_key, o.uniform)) {
        ++i;
        if (i % 5000 == 0) pelapsed("Processed " + std::to_string(i) + " variants", true);
        if (last_seq_name.empty()) {
            last_seq_name = v.seq_name;
            if (used) used->push_back(last_seq_name);
        }
        if (for_index ? (!v.has_alts || !v.is_present) : !v.has_alts) continue;
        if (vb.empty()) {
            vb.add(std::move(v));
            continue;
        }
        if (!vb.near_to_last(v) || last_seq_name != v.seq_name) {
            on_block(vb, last_seq_name, ref_of(last_seq_name));
            vb.clear();
            if (last_seq_name != v.seq_name) {
                last_seq_name = v.seq_name;
                if (used) used->push_back(last_seq_name);
            }
        }
        vb.add(std::move(v));
    }
    if (!vb.empty()) {
        on_block(vb, last_seq_name, ref_of(last_seq_name));
        vb.clear();
    }
    return i;
}

// ---- index file (index_file.hpp): payload out of / into the contexts ---------------------------------------------------
void save_index(Device &dev, const Options &o)
{
    IndexPayload p;
    const int which[2] = {MG_BF_CTX, MG_BF_ALT}; // payload order of main.cpp:409-411: context_bf, bf, ref_bf
    for (int i = 0; i < 2; ++i) {
        uint64_t size, nset;
        int mode;
        dev.check(mg_bf_info(dev.ctx, which[i], &size, &nset, &mode), "mg_bf_info");
        p.filt[i].mode = (uint64_t)mode;
        p.filt[i].pos.resize(nset);
        p.filt[i].cnt.resize(nset);
        dev.check(mg_bf_export_sparse(dev.ctx, which[i], p.filt[i].pos.data(), p.filt[i].cnt.data()), "mg_bf_export_sparse");
    }
    uint64_t nkeys = 0;
    dev.check(mg_map_size(dev.ctx, &nkeys), "mg_map_size");
    p.stride = STRIDE;
    p.rows.resize(nkeys * STRIDE);
    p.vals.resize(nkeys);
    if (nkeys) dev.check(mg_map_export(dev.ctx, p.rows.data(), STRIDE, p.vals.data()), "mg_map_export");
    // Both containers by default: the reference's (.zst: one zstd stream over the filters' full bit vectors -- gigabytes of
    // zeros through a single-threaded codec, ~1.5 s to write and ~1.2 s to read at -b 4) for the reference's own binary, and
    // this build's sparse one (.hipz, milliseconds), which `call` prefers while it is not older than the .zst beside it.
    // MALVA_GENO_INDEX_FORMAT=zst | hipz writes one of them only.  Each is written under a temporary name and renamed: a run
    // that dies mid-write leaves no truncated index for `call` to find.
    const char *fmt = getenv("MALVA_GENO_INDEX_FORMAT");
    const std::string want = fmt ? fmt : "both";
    if (want != "both" && want != "zst" && want != "hipz") throw std::runtime_error("MALVA_GENO_INDEX_FORMAT: zst, hipz or both");
    auto write_zst = [&]() {
        const std::string final_path = index_path(o, ".zst");
        if (want == "hipz") {
            unlink(final_path.c_str()); // no stale index of the other kind beside the new one
            return;
        }
        const std::string tmp_path = final_path + ".tmp." + std::to_string((long)getpid());
        try {
            Timed t("index file: .zst");
            save_index_zst(tmp_path, p, o.bf_size);
        } catch (...) {
            unlink(tmp_path.c_str());
            throw;
        }
        if (rename(tmp_path.c_str(), final_path.c_str()) != 0) {
            unlink(tmp_path.c_str());
            throw std::runtime_error("cannot write " + final_path);
        }
    };
    // side by side (the .zst takes seconds, single-threaded inside libzstd); the .hipz is renamed into place after the .zst,
    // so it is the newer file of the two
    auto zst_job = std::async(std::launch::async, write_zst);
    std::exception_ptr hipz_err;
    const std::string hipz_final = index_path(o, ".hipz"), hipz_tmp = hipz_final + ".tmp." + std::to_string((long)getpid());
    if (want == "zst") unlink(hipz_final.c_str());
    else {
        try {
            Timed t("index file: .hipz");
            save_index_hipz(hipz_tmp, p, o.k, o.ref_k, o.bf_size, hipz::panel_tie_of(o.vcf_path));
        } catch (...) {
            unlink(hipz_tmp.c_str());
            hipz_err = std::current_exception();
        }
    }
    try {
        zst_job.get();
    } catch (...) {
        unlink(hipz_tmp.c_str());
        throw;
    }
    if (hipz_err) std::rethrow_exception(hipz_err);
    if (want != "zst") {
        if (rename(hipz_tmp.c_str(), hipz_final.c_str()) != 0) {
            unlink(hipz_tmp.c_str());
            throw std::runtime_error("cannot write " + hipz_final);
        }
        utimensat(AT_FDCWD, hipz_final.c_str(), nullptr, 0); // (a rename keeps the time of the last write, which was before the .zst's)
    }
}

// every device of a multi-GPU call holds the whole index (the read-only structures are replicated):
// the file is read once and imported into all contexts side by side
template <class F> void on_all_devices(std::vector<Device> &devs, F f)
{
    if (devs.size() == 1) return f(devs[0], 0);
    std::vector<std::exception_ptr> errs(devs.size());
    std::vector<std::thread> pool;
    for (size_t d = 0; d < devs.size(); ++d)
        pool.emplace_back([&, d]() {
            try {
                f(devs[d], d);
            } catch (...) {
                errs[d] = std::current_exception();
            }
        });
    for (auto &t : pool) t.join();
    for (auto &e : errs)
        if (e) std::rethrow_exception(e);
}

// the index file -> payload (host only: runs beside the devices' start-up), then payload -> every context
void read_index(const Options &o, IndexPayload &p)
{
    Timed t("startup: index file -> payload");
    const std::string zst = index_path(o, ".zst"), hipz = index_path(o, ".hipz");
    struct stat sz, sh;
    const bool has_zst = stat(zst.c_str(), &sz) == 0, has_hipz = stat(hipz.c_str(), &sh) == 0;
    auto newer = [](const struct stat &a, const struct stat &b) { // a strictly newer than b
        return a.st_mtim.tv_sec != b.st_mtim.tv_sec ? a.st_mtim.tv_sec > b.st_mtim.tv_sec : a.st_mtim.tv_nsec > b.st_mtim.tv_nsec;
    };
    // the sparse container unless the reference's one is newer (an index brought over from the reference's binary) -- or unless the
    // sparse one says it was built from another panel than the VCF given here (its header holds that VCF's size and modification
    // time: file dates alone do not survive a copy or a restore) while the reference's container is there to be read instead
    bool stale = false;
    if (has_hipz && has_zst) {
        const hipz::PanelTie tie = index_hipz_tie(hipz);
        stale = tie.known() && !(tie == hipz::panel_tie_of(o.vcf_path));
        if (stale) std::cerr << "[malva-geno] " << hipz << " was built from another version of " << o.vcf_path << ": reading " << zst << std::endl;
    }
    if (has_hipz && !stale && !(has_zst && newer(sz, sh))) load_index_hipz(hipz, p, o.k, o.ref_k, o.bf_size, STRIDE);
    else if (has_zst) load_index_zst(zst, p, o.bf_size, STRIDE);
    else throw std::runtime_error("cannot open index " + index_path(o, ".zst") + " (run `malva-geno index` with the same -k -r -b first)");
}
void import_index(std::vector<Device> &devs, const Options &o, const IndexPayload &p)
{
    Timed t("startup: payload -> device");
    on_all_devices(devs, [&](Device &dev, size_t) {
        const int which[2] = {MG_BF_CTX, MG_BF_ALT};
        for (int i = 0; i < 2; ++i)
            dev.check(mg_bf_import_sparse(dev.ctx, which[i], (int)p.filt[i].mode, o.bf_size, p.filt[i].pos.data(), p.filt[i].cnt.data(), p.filt[i].pos.size()),
                      "mg_bf_import_sparse");
        if (!p.vals.empty()) dev.check(mg_map_import(dev.ctx, p.rows.data(), STRIDE, p.vals.size(), p.vals.data()), "mg_map_import");
    });
}

// ---------------------------------------------------------------------------------------------------------------
int index_main(const Options &o)
{
    Reference refs;
    if (!read_fasta(o.fasta_path, o.strip_chr, refs)) {
        std::cerr << "ERROR: cannot open " << o.fasta_path << std::endl;
        return 1;
    }
    VcfReader vcf(o.vcf_path, o.samples);
    if (!vcf.ok()) {
        std::cerr << vcf.error << std::endl;
        return 1;
    }
    vcf.defer_genotypes = device_gt_wanted(vcf) && !getenv("MALVA_GENO_HOST_CUT"); // (the decode rides on the device cutter's batches)
    vcf.decode_ahead(o.freq_key, o.uniform);
    pelapsed("Reference processed");
    Device dev;
    if (mg_create(&dev.ctx, o.device, o.k, o.ref_k, o.bf_size) != MG_OK) {
        std::cerr << "ERROR: no usable MI355X/HIP device " << o.device << " (or not enough memory for two filters of " << o.bf_size
                  << " bits); this build has no CPU path" << std::endl;
        return 1;
    }
    Rows ref_rows, alt_rows;
    auto flush = [&](bool force) {
        if (ref_rows.n && (force || ref_rows.n >= (1u << 20))) {
            dev.check(mg_map_insert(dev.ctx, ref_rows.data.data(), STRIDE, ref_rows.n), "mg_map_insert");
            ref_rows.clear();
        }
        if (alt_rows.n && (force || alt_rows.n >= (1u << 20))) {
            dev.check(mg_bf_insert(dev.ctx, MG_BF_ALT, alt_rows.data.data(), STRIDE, alt_rows.n), "mg_bf_insert");
            alt_rows.clear();
        }
    };
    std::vector<std::string> used;
    // General blocks are enumerated ON THE DEVICE, a few thousand at a time (mg_index_blocks: chains, distinct haplotype
    // picks, signature assembly, exact-map insert / filter bit -- extract_kmers + add_kmers_to_bf, main.cpp:349-350);
    // blocks the device hands back (a capacity exceeded, a window clipped by a contig end, a REF k-mer with a base
    // outside ACGT) are enumerated by all host cores and inserted through the batch calls.
    std::map<std::string, uint64_t> contig_base;
    {
        const std::string all = concat_reference(refs, contig_base);
        dev.check(mg_reference_upload(dev.ctx, all.data(), all.size()), "mg_reference_upload");
    }
    const bool host_only = o.k > MG_MAX_PACKED_K || getenv("MALVA_GENO_HOST_ENUM"); // the variable forces the host enumerator (tests)
    std::vector<Block> waiting;
    std::vector<const std::string *> waiting_ref;
    std::vector<uint64_t> waiting_base;
    size_t waiting_cells = 0, n_host_blocks = 0, n_general_blocks = 0;
    auto enumerate_waiting = [&]() {
        const size_t nb = waiting.size();
        if (!nb) return;
        n_general_blocks += nb;
        std::vector<uint8_t> redo(nb, host_only ? 1 : 0);
        if (!host_only) {
            BlockArrays ba;
            for (size_t b = 0; b < nb; ++b) {
                ba.open_block(waiting_base[b], waiting_ref[b]->size());
                for (const Variant &v : waiting[b].vars) ba.add(v);
                ba.close_block();
            }
            const bool device_ok = !ba.wide_alleles;
            const size_t nv = ba.ipos.size();
            const uint32_t n_samples = (uint32_t)vcf.keep.size();
            const PanelGenotypes pg = pack_genotypes(waiting, nv, n_samples, o.haploid);
            std::vector<uint8_t> overflow(nv, 1);
            if (device_ok) {
                const mg_blocks_host x = ba.view(pg, n_samples);
                dev.check(mg_index_blocks(dev.ctx, &x, o.haploid, overflow.data()), "mg_index_blocks");
            }
            for (size_t b = 0; b < nb; ++b)
                for (uint32_t v = ba.blk_var_off[b]; v < ba.blk_var_off[b + 1]; ++v) redo[b] = redo[b] || overflow[v];
        }
        std::vector<size_t> todo;
        for (size_t b = 0; b < nb; ++b)
            if (redo[b]) todo.push_back(b);
        n_host_blocks += todo.size();
        const size_t nt = todo.size();
        std::vector<std::vector<AlleleSignatures>> sigs(nt);
        const unsigned n_threads = (unsigned)std::max<size_t>(1, std::min<size_t>({(size_t)std::thread::hardware_concurrency(), 16, std::max<size_t>(nt, 1)}));
        std::vector<std::exception_ptr> errs(n_threads);
        std::vector<size_t> err_at(n_threads, SIZE_MAX);
        std::vector<std::thread> pool_t;
        for (unsigned t = 0; t < n_threads && nt; ++t)
            pool_t.emplace_back([&, t]() {
                for (size_t q = t; q < nt; q += n_threads) {
                    try {
                        genotypes_from_entries(waiting[todo[q]]);
                        sigs[q] = waiting[todo[q]].extract(*waiting_ref[todo[q]], o.haploid); // main.cpp:349
                    } catch (...) {
                        errs[t] = std::current_exception();
                        err_at[t] = q;
                        return;
                    }
                }
            });
        for (auto &th : pool_t) th.join();
        size_t first = SIZE_MAX;
        for (unsigned t = 0; t < n_threads; ++t)
            if (errs[t] && (first == SIZE_MAX || err_at[t] < err_at[first])) first = t;
        if (first != SIZE_MAX) std::rethrow_exception(errs[first]);
        for (size_t q = 0; q < nt; ++q) {
            for (const auto &per_allele : sigs[q]) // add_kmers_to_bf, main.cpp:122-144
                for (const auto &as : per_allele)
                    for (const auto &sig : as.second)
                        for (const auto &kmer : sig) (as.first == 0 ? ref_rows : alt_rows).add(kmer);
            flush(false);
        }
        waiting.clear();
        waiting_ref.clear();
        waiting_base.clear();
        waiting_cells = 0;
    };
    // Blocks of one variant whose alleles are all shorter than k -- nearly every block of a SNP panel -- are indexed ON THE
    // DEVICE too, a batch at a time (mg_index_isolated: signature assembly from the uploaded reference, exact-map insert /
    // filter bit); the host keeps the few the device hands back (a base outside ACGT in the window) and those whose
    // right flank a contig end clips (the reference then makes a shorter k-mer, var_block.hpp:187).
    struct LoneBatch : LoneArrays {
        std::vector<Block> blocks; // kept for the variants handed back
        std::vector<const std::string *> refs;
        size_t cells = 0;
    } lone;
    size_t n_lone_device = 0, n_lone_host = 0;
    auto index_lone = [&]() {
        if (!lone.n()) return;
        std::vector<uint8_t> overflow(lone.n(), 1);
        dev.check(mg_index_isolated(dev.ctx, lone.n(), lone.pos.data(), lone.var_allele_off.data(), lone.allele_off.data(), lone.pool.data(), lone.pool.size(),
                                    lone.present.data(), lone.flags.data(), overflow.data()),
                  "mg_index_isolated");
        for (size_t v = 0; v < lone.n(); ++v) {
            if (!overflow[v]) {
                ++n_lone_device;
                continue;
            }
            ++n_lone_host;
            genotypes_from_entries(lone.blocks[v]);
            lone.blocks[v].extract_lone(*lone.refs[v], o.haploid, [&](int a, const std::string &kmer) { (a == 0 ? ref_rows : alt_rows).add(kmer); });
            flush(false);
        }
        lone = LoneBatch();
    };
    const size_t n = for_each_block(vcf, o, refs, true, &used, [&](Block &vb, const std::string &seq_name, const std::string &reference) {
        if (vb.is_lone_short()) {
            const Variant &v = vb.vars[0];
            const bool on_device = !host_only && contig_base.count(seq_name) && v.n_alleles() <= 64 && right_flank_fits(v, o.k, reference.size());
            if (!on_device) { // one k-mer per carried allele, no containers
                genotypes_from_entries(vb);
                vb.extract_lone(reference, o.haploid, [&](int a, const std::string &kmer) { (a == 0 ? ref_rows : alt_rows).add(kmer); });
                flush(false);
                return;
            }
            lone.add(v, contig_base.at(seq_name), o.k, reference.size(), o.haploid);
            lone.cells += v.n_genotypes();
            lone.refs.push_back(&reference);
            lone.blocks.push_back(std::move(vb));
            vb = Block((int)o.k);
            if (lone.n() >= 200000 || lone.cells >= (200u << 20)) index_lone();
            return;
        }
        auto cb = contig_base.find(seq_name);
        waiting_base.push_back(cb == contig_base.end() ? 0 : cb->second);
        waiting_ref.push_back(&reference);
        for (const Variant &v : vb.vars) waiting_cells += v.n_genotypes();
        waiting.push_back(std::move(vb));
        vb = Block((int)o.k);
        if (waiting.size() >= 4096 || waiting_cells >= (200u << 20)) enumerate_waiting(); // bound the panel genotypes held in memory
    }, &dev);
    enumerate_waiting();
    index_lone();
    flush(true);
    if (n_lone_device + n_lone_host)
        std::cerr << "[malva-geno] " << n_lone_device + n_lone_host << " lone variant(s): " << n_lone_device << " indexed on the device, " << n_lone_host
                  << " on the host" << std::endl;
    if (n_general_blocks)
        std::cerr << "[malva-geno] " << n_general_blocks << " general block(s): " << n_general_blocks - n_host_blocks << " enumerated on the device, " << n_host_blocks
                  << " on the host" << std::endl;
    pelapsed("Processed " + std::to_string(n) + " variants");
    dev.check(mg_bf_finalize(dev.ctx, MG_BF_ALT), "mg_bf_finalize(bf)"); // main.cpp:378
    pelapsed("BF creation complete");
    for (const auto &name : used) { // main.cpp:383-401
        auto it = refs.seqs.find(name);
        static const std::string empty;
        const std::string &seq = it == refs.seqs.end() ? empty : it->second;
        auto cb = contig_base.find(name);
        if (cb != contig_base.end()) // the contig is already in HBM (mg_reference_upload above): nothing crosses PCIe again
            dev.check(mg_ref_scan_resident(dev.ctx, cb->second, seq.size()), "mg_ref_scan_resident");
        else
            dev.check(mg_ref_scan(dev.ctx, seq.data(), seq.size()), "mg_ref_scan");
    }
    pelapsed("Reference BF creation complete");
    dev.check(mg_bf_finalize(dev.ctx, MG_BF_CTX), "mg_bf_finalize(context_bf)"); // main.cpp:404
    save_index(dev, o);
    return 0;
}

// ---- call -----------------------------------------------------------------------------------------------------
// k-mer table: text dump, `KMER count` per line -> SoA 2-bit table in pieces
struct TablePiece {
    std::vector<uint64_t> hi, lo;
    std::vector<uint32_t> cnt;
    void clear()
    {
        hi.clear();
        lo.clear();
        cnt.clear();
    }
};

// Rows with a symbol outside ACGT (KMC never lists any) go through the exact ASCII calls at the end.
struct OddRows {
    Rows ctx, kmer;
    std::vector<uint32_t> cnt;
};
// One line of the dump, [p, e) without its terminator: `KMER<ws>count`.  main.cpp:491 upper-cases the k-mer.
inline void parse_table_line(const char *p, const char *e, const Options &o, TablePiece &t, OddRows &odd)
{
    static const struct Lut {
        int8_t code[256];
        Lut()
        {
            for (int i = 0; i < 256; ++i) code[i] = -1;
            code['A'] = code['a'] = 0;
            code['C'] = code['c'] = 1;
            code['G'] = code['g'] = 2;
            code['T'] = code['t'] = 3;
        }
    } lut;
    if (e > p && e[-1] == '\r') --e;
    if (p == e) return;
    const char *q = p;
    uint64_t hi = 0, lo = 0;
    bool acgt = true;
    while (q < e && !isspace((unsigned char)*q)) {
        const int c = lut.code[(unsigned char)*q++];
        acgt = acgt && c >= 0;
        hi = (hi << 2) | (lo >> 62);
        lo = (lo << 2) | (uint64_t)(c & 3);
    }
    const size_t len = (size_t)(q - p);
    if (len != o.ref_k) throw std::runtime_error("k-mer table holds a " + std::to_string(len) + "-mer, expected -r " + std::to_string(o.ref_k));
    while (q < e && isspace((unsigned char)*q)) ++q;
    uint64_t count = 0; // strtoul: leading digits
    while (q < e && *q >= '0' && *q <= '9') count = count * 10 + (uint64_t)(*q++ - '0');
    if (!acgt || o.ref_k > MG_MAX_PACKED_K) { // (a row the 2-bit table cannot hold -- or any row, beyond 64 bases: the ASCII batch forms below)
        std::string ctx(p, len);
        upper_inplace(ctx);
        odd.ctx.add(ctx);
        odd.kmer.add(ctx.substr((o.ref_k - o.k) / 2, o.k));
        odd.cnt.push_back((uint32_t)count);
        return;
    }
    t.hi.push_back(hi);
    t.lo.push_back(lo);
    t.cnt.push_back((uint32_t)count);
}

// The dump of a whole-genome sample is >100 GB of text: a plain (uncompressed) file is mapped and parsed by all
// host cores, 64 MiB of text per task (a line belongs to the task that holds its first byte), and the parsed
// pieces are scanned by THIS thread in whatever order they complete -- the counter updates commute.  A
// compressed dump is inflated and parsed by one thread.
//
// With several GPUs the table shards by rows: every device has a consumer thread that takes the next parsed piece
// and scans it into ITS context's counters; one all-reduce over RCCL then makes every device hold the whole
// table's counters.
void scan_table(std::vector<Device> &devs, const Options &o, const std::string &path)
{
    std::atomic<uint64_t> total{0};
    OddRows odd;
    Device &dev = devs[0];
    auto scan_piece_on = [&](Device &d, TablePiece &t) {
        if (!t.cnt.empty()) d.check(mg_kmc_scan(d.ctx, t.hi.data(), t.lo.data(), t.cnt.data(), t.cnt.size()), "mg_kmc_scan");
        total += t.cnt.size();
        t.clear();
    };
    bool gz = false;
    {
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("cannot open " + path);
        unsigned char m[2] = {0, 0};
        gz = fread(m, 1, 2, f) == 2 && m[0] == 0x1f && m[1] == 0x8b;
        fclose(f);
    }
    struct stat st;
    if (!gz && stat(path.c_str(), &st) == 0 && st.st_size > 0) {
        const size_t size = (size_t)st.st_size;
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) throw std::runtime_error("cannot open " + path);
        const char *base = (const char *)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (base == MAP_FAILED) throw std::runtime_error("cannot map " + path);
        madvise((void *)base, size, MADV_SEQUENTIAL);
        const char *tb = getenv("MALVA_GENO_TABLE_TASK"); // bytes of text per parsing task (tests shrink it to cross many boundaries)
        const size_t task_bytes = tb && atol(tb) > 0 ? (size_t)atol(tb) : (64u << 20), n_tasks = (size + task_bytes - 1) / task_bytes;
        const unsigned n_threads = (unsigned)std::max<size_t>(1, std::min<size_t>({(size_t)std::thread::hardware_concurrency(), 16, n_tasks}));
        std::atomic<size_t> next_task{0};
        std::mutex mu;
        std::condition_variable cv;
        std::deque<TablePiece> done;   // parsed, waiting for the device
        size_t finished_threads = 0;
        std::string error;
        auto worker = [&]() {
            TablePiece t;
            OddRows mine;
            try {
                for (;;) {
                    const size_t task = next_task.fetch_add(1);
                    if (task >= n_tasks) break;
                    const char *lim = base + std::min(size, (task + 1) * task_bytes), *end = base + size;
                    const char *p = base + task * task_bytes;
                    if (task) { // skip the line that started in the previous task
                        const char *nl = (const char *)memchr(p - 1, '\n', (size_t)(end - (p - 1)));
                        p = nl ? nl + 1 : end;
                    }
                    while (p < lim) {
                        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
                        const char *e = nl ? nl : end;
                        parse_table_line(p, e, o, t, mine);
                        p = e + 1;
                    }
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return done.size() < 2 * n_threads || !error.empty(); }); // bound what is in flight
                    done.emplace_back(std::move(t));
                    t = TablePiece();
                    cv.notify_all();
                }
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lk(mu);
                if (error.empty()) error = e.what();
            }
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < mine.cnt.size(); ++i) {
                odd.ctx.add(std::string(&mine.ctx.data[i * STRIDE]));
                odd.kmer.add(std::string(&mine.kmer.data[i * STRIDE]));
                odd.cnt.push_back(mine.cnt[i]);
            }
            ++finished_threads;
            cv.notify_all();
        };
        std::vector<std::thread> pool;
        for (unsigned i = 0; i < n_threads; ++i) pool.emplace_back(worker);
        auto consumer = [&](Device &d) { // one per device; this thread is device 0's
            for (;;) {
                TablePiece t;
                bool failed;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return !done.empty() || finished_threads == n_threads; });
                    if (done.empty()) break;
                    t = std::move(done.front());
                    done.pop_front();
                    failed = !error.empty();
                    cv.notify_all();
                }
                try {
                    if (!failed) scan_piece_on(d, t);
                } catch (const std::exception &e) {
                    std::lock_guard<std::mutex> lk(mu);
                    if (error.empty()) error = e.what();
                    cv.notify_all();
                }
            }
        };
        std::vector<std::thread> consumers;
        for (size_t d = 1; d < devs.size(); ++d) consumers.emplace_back([&, d]() { consumer(devs[d]); });
        consumer(devs[0]);
        for (auto &th : consumers) th.join();
        for (auto &th : pool) th.join();
        munmap((void *)base, size);
        if (!error.empty()) throw std::runtime_error(error);
    } else {
        LineReader in(path);
        if (!in.ok()) throw std::runtime_error("cannot open " + path);
        TablePiece t;
        std::string line;
        const size_t piece = 1u << 24;
        size_t turn = 0; // one inflating thread: the pieces still go round the devices, so the exchange is exercised
        while (in.next(line)) {
            parse_table_line(line.data(), line.data() + line.size(), o, t, odd);
            if (t.cnt.size() == piece) scan_piece_on(devs[turn++ % devs.size()], t);
        }
        scan_piece_on(devs[turn % devs.size()], t);
    }
    total += odd.cnt.size();
    if (odd.cnt.size()) { // main.cpp:495-499 through the ASCII batch calls
        std::vector<int32_t> ic(odd.cnt.begin(), odd.cnt.end());
        dev.check(mg_map_increment(dev.ctx, odd.kmer.data.data(), STRIDE, odd.kmer.n, ic.data()), "mg_map_increment");
        std::vector<uint8_t> in_ctx(odd.cnt.size());
        dev.check(mg_bf_test(dev.ctx, MG_BF_CTX, odd.ctx.data.data(), STRIDE, odd.ctx.n, in_ctx.data()), "mg_bf_test");
        Rows pass;
        std::vector<uint32_t> pc;
        for (size_t i = 0; i < odd.cnt.size(); ++i)
            if (!in_ctx[i]) {
                pass.add(std::string(&odd.kmer.data[i * STRIDE]));
                pc.push_back(odd.cnt[i]);
            }
        if (pass.n) dev.check(mg_bf_increment(dev.ctx, MG_BF_ALT, pass.data.data(), STRIDE, pass.n, pc.data()), "mg_bf_increment");
        // device 0's counters join the all-reduce below; exact-map keys the packed table cannot hold live in a host
        // list inside each context, which no collective reaches: the other devices get those increments directly
        Rows irr;
        std::vector<int32_t> irr_c;
        for (size_t i = 0; i < odd.cnt.size(); ++i) {
            const std::string kmer(&odd.kmer.data[i * STRIDE]);
            if (kmer.find_first_not_of("ACGT") != std::string::npos) {
                irr.add(kmer);
                irr_c.push_back((int32_t)odd.cnt[i]);
            }
        }
        for (size_t d = 1; d < devs.size() && irr.n; ++d)
            devs[d].check(mg_map_increment(devs[d].ctx, irr.data.data(), STRIDE, irr.n, irr_c.data()), "mg_map_increment");
    }
    if (devs.size() > 1) { // the exchange step: ncclAllReduce(sum, uint32) of [bf counters | map counters] on every device
        std::vector<mg_ctx *> ctxs;
        for (auto &d : devs) ctxs.push_back(d.ctx);
        dev.check(mg_counters_allreduce_all(ctxs.data(), (int)ctxs.size()), "mg_counters_allreduce_all");
        for (auto &d : devs) d.check(mg_synchronize(d.ctx), "mg_synchronize");
    }
    std::cerr << "[malva-geno] scanned " << total << " k-mers" << (devs.size() > 1 ? " on " + std::to_string(devs.size()) + " devices" : std::string()) << std::endl;
}

// The KMC database itself (main.cpp:444-449, 482-490): the prefix table goes to every device once, then each device
// takes a contiguous range of the records, straight out of the mapped <db>.kmc_suf -- the host decodes nothing; the
// library uploads the raw records in pieces beside the scan of the previous piece and rebuilds the k-mers on the device.
void scan_kmc_db(std::vector<Device> &devs, const Options &o, const std::string &prefix)
{
    KmcDb db;
    db.open(prefix);
    if (db.k != o.ref_k) throw std::runtime_error("KMC database holds " + std::to_string(db.k) + "-mers, expected -r " + std::to_string(o.ref_k));
    std::cerr << "[malva-geno] KMC database: " << db.total << " " << db.k << "-mers, counts " << db.min_count << ".." << db.max_count << ", "
              << db.lut.size() / (1ULL << (2 * db.lut_prefix_len)) << " bin(s) x 4^" << db.lut_prefix_len << " prefixes, " << db.rec_bytes << " B/record" << std::endl;
    on_all_devices(devs, [&](Device &d, size_t i) {
        d.check(mg_kmc_set_lut(d.ctx, db.lut.data(), db.lut.size(), db.lut_prefix_len, db.suffix_bytes, db.counter_size, db.min_count, db.max_count, db.total),
                "mg_kmc_set_lut");
        const uint64_t a = db.total * i / devs.size(), b = db.total * (i + 1) / devs.size();
        if (b > a) d.check(mg_kmc_scan_records(d.ctx, db.records + a * db.rec_bytes, b - a, a), "mg_kmc_scan_records");
    });
    if (devs.size() > 1) {
        std::vector<mg_ctx *> ctxs;
        for (auto &d : devs) ctxs.push_back(d.ctx);
        devs[0].check(mg_counters_allreduce_all(ctxs.data(), (int)ctxs.size()), "mg_counters_allreduce_all");
        for (auto &d : devs) d.check(mg_synchronize(d.ctx), "mg_synchronize");
    }
    std::cerr << "[malva-geno] scanned " << db.total << " k-mers" << (devs.size() > 1 ? " on " + std::to_string(devs.size()) + " devices" : std::string()) << std::endl;
}

// The sample's reads, counted on the devices (the KMC step of MALVA:104-110, mg_reads_*): one reader thread per file fills pinned
// chunks of whole records; every chunk goes to EVERY device, each counting only its own partition of the keys (part = its
// rank), so a k-mer's count is whole on one device before --min-count applies; the exchange then sums the counters.
void count_reads(std::vector<Device> &devs, const Options &o, const std::vector<std::string> &files)
{
    const uint32_t n = (uint32_t)devs.size();
    for (uint32_t d = 0; d < n; ++d) devs[d].check(mg_reads_begin(devs[d].ctx, o.min_count, o.max_count, d, n), "mg_reads_begin");
    ReadsChunker ch;
    ch.ref_k = o.ref_k;
    if (const char *cb = getenv("MALVA_GENO_READS_CHUNK")) // bytes per chunk (tests shrink it to split records across chunks)
        if (atol(cb) > 0) ch.chunk_bytes = std::max<size_t>((size_t)atol(cb), 2 * o.ref_k + 4096);
    ch.alloc = [](size_t bytes) -> void * {
        void *p = nullptr;
        return mg_host_alloc(&p, bytes) == MG_OK ? p : nullptr;
    };
    ch.release = [](void *p) { mg_host_free(p); };
    uint64_t bytes = 0;
    {
        Timed t("reads: read + upload");
        ch.run(files, [&](const char *buf, size_t len) {
            for (auto &d : devs) d.check(mg_reads_add(d.ctx, buf, len), "mg_reads_add");
            bytes += len;
        });
    }
    uint64_t kept = 0;
    {
        Timed t("reads: count + scan");
        std::vector<uint64_t> k(n, 0);
        on_all_devices(devs, [&](Device &d, size_t i) { d.check(mg_reads_finish(d.ctx, &k[i]), "mg_reads_finish"); });
        for (auto v : k) kept += v;
    }
    float ms[5] = {0, 0, 0, 0, 0};
    uint64_t cn[5] = {0, 0, 0, 0, 0};
    devs[0].check(mg_reads_stats(devs[0].ctx, ms, cn), "mg_reads_stats");
    if (g_timers.on) { // device time of device 0's phases (HIP events)
        const char *names[5] = {"reads device: pack", "reads device: window+filter", "reads device: file", "reads device: reduce", "reads device: scan"};
        for (int i = 0; i < 5; ++i) g_timers.add(names[i], ms[i] / 1000.0);
    }
    if (devs.size() > 1) {
        std::vector<mg_ctx *> ctxs;
        for (auto &d : devs) ctxs.push_back(d.ctx);
        devs[0].check(mg_counters_allreduce_all(ctxs.data(), (int)ctxs.size()), "mg_counters_allreduce_all");
        for (auto &d : devs) d.check(mg_synchronize(d.ctx), "mg_synchronize");
    }
    std::cerr << "[malva-geno] counted " << cn[1] << " " << o.ref_k << "-mer windows of " << files.size() << " read file(s) (" << bytes
              << " bytes), " << cn[2] << " through the gate, " << kept << " k-mers kept (count " << std::max<uint32_t>(o.min_count, 1) << ".."
              << o.max_count << ", " << cn[3] << " pass(es))" << (devs.size() > 1 ? " on " + std::to_string(devs.size()) + " devices" : std::string()) << std::endl;
}

int call_main(const Options &o)
{
    // Start-up runs three things side by side: the FASTA (host), the index file (host) and the devices (HIP start-up is
    // ~0.4 s by itself).  The sample's table is scanned as soon as the index is on the device; the reference joins after it.
    Reference refs;
    auto fasta_read = std::async(std::launch::async, [&]() {
        Timed t("startup: FASTA");
        return read_fasta(o.fasta_path, o.strip_chr, refs);
    });
    IndexPayload payload;
    auto index_read = std::async(std::launch::async, [&]() { read_index(o, payload); });
    auto start_vcf = [&](VcfReader &r) {
        if (r.ok()) {
            r.want_prefix = true;
            r.defer_genotypes = device_gt_wanted(r) && !getenv("MALVA_GENO_HOST_CUT"); // (the decode rides on the device cutter's batches)
            r.decode_ahead(o.freq_key, o.uniform);
        }
    };
    std::unique_ptr<VcfReader> vcf_first(new VcfReader(o.vcf_path, o.samples)); // (a panel of any size is decoded by a pool of threads: started here, it works through start-up)
    start_vcf(*vcf_first);
    auto fail_early = [&](const std::string &msg) { // (the readers hold references to this frame: let them finish first)
        fasta_read.wait();
        index_read.wait();
        std::cerr << msg << std::endl;
        return 1;
    };
    // the sample's k-mers: the KMC database the reference opens (main.cpp:444-449), or -- when there is none -- a text dump
    // or the reads themselves, counted on the devices (MALVA:104-110).  --cohort: a manifest of such inputs, all of them
    // resolved and checked here, before any device exists and before anything is written.
    std::vector<CohortSample> samples;
    try {
        if (o.cohort) samples = read_cohort_manifest(o.kmc_path, o.ref_k, MG_MAX_PACKED_K);
        else samples.push_back({std::string(), resolve_sample_input(o.kmc_path, o.ref_k, MG_MAX_PACKED_K)});
    } catch (const std::exception &e) {
        return fail_early(e.what());
    }
    if (o.priors.on) { // (the sizes already tell: before any device is created, before anything is written)
        const std::string why = o.priors.groups ? prior_groups_error(samples.size()) : prior_group_error(samples.size(), o.cohort_group);
        if (!why.empty()) return fail_early("ERROR: " + why);
    }
    // --gpus N: one context per device -d .. -d+N-1.  MALVA_GENO_SHARE_DEVICE=1 puts all N contexts on device -d: the
    // N-way layout (sharded scan, exchange, split genotyping) rehearsed on a one-GPU box, the exchange then being a
    // kernel instead of RCCL (which rejects two ranks on one device).
    const bool share_device = getenv("MALVA_GENO_SHARE_DEVICE") && atoi(getenv("MALVA_GENO_SHARE_DEVICE")) != 0;
    std::vector<Device> devs((size_t)o.gpus);
    {
        Timed t("startup: devices");
        for (int d = 0; d < o.gpus; ++d)
            if (mg_create(&devs[(size_t)d].ctx, share_device ? o.device : o.device + d, o.k, o.ref_k, o.bf_size) != MG_OK)
                return fail_early("ERROR: no usable MI355X/HIP device " + std::to_string(share_device ? o.device : o.device + d) + "; this build has no CPU path");
    }
    if (o.gpus > 1) {
        std::vector<mg_ctx *> ctxs;
        for (auto &d : devs) ctxs.push_back(d.ctx);
        devs[0].check(mg_comm_init_all(ctxs.data(), o.gpus), "mg_comm_init_all");
        int backend = MG_COMM_NONE;
        mg_comm_info(devs[0].ctx, nullptr, nullptr, &backend);
        std::cerr << "[malva-geno] " << o.gpus << " contexts, exchange: " << (backend == MG_COMM_RCCL ? "RCCL all-reduce" : "one device, kernel sum") << std::endl;
    }
    try {
        index_read.get();
    } catch (...) {
        fasta_read.wait();
        throw;
    }
    import_index(devs, o, payload);
    payload = IndexPayload();
    pelapsed("Reference processed"); // (the phase names are the reference's, main.cpp:452-470; the FASTA itself may still be on its way)
    auto scan_sample = [&](const SampleInput &in) {
        if (in.kind == SampleInput::READS) count_reads(devs, o, in.reads); // MALVA:104-110 + main.cpp:482-500
        else if (in.kind == SampleInput::KMC_DB) scan_kmc_db(devs, o, in.path); // main.cpp:482-500
        else scan_table(devs, o, in.path);
    };
    if (!o.cohort) {
        Timed t("startup: table scan");
        scan_sample(samples[0].input);
    }
    pelapsed("BF weights created");
    if (!fasta_read.get()) {
        std::cerr << "ERROR: cannot open " << o.fasta_path << std::endl;
        return 1;
    }

    // concatenated reference for the fused isolated path
    std::map<std::string, uint64_t> contig_base;
    {
        const std::string all = concat_reference(refs, contig_base);
        Timed t("startup: reference upload");
        on_all_devices(devs, [&](Device &d, size_t) { d.check(mg_reference_upload(d.ctx, all.data(), all.size()), "mg_reference_upload"); });
    }
    CallTimes times;                          // the batch calls' device time, all passes (the workers' batch by batch, added as their text is taken)
    const bool want_sample = !o.sample_stats.empty(); // --sample-stats: the batches carry their alleles' classes
    PriorsFile priors_file;                   // --priors-out
    MergedFormat merged_fmt;                  // --merged-format bcf | ubcf
    merged_fmt.bcf_out = !o.merged.empty() && !o.merged_format.empty() && o.merged_format != "vcf", merged_fmt.bcf_bgzf = o.merged_format == "bcf";
    const bool bcf_out = merged_fmt.bcf_out, bcf_bgzf = merged_fmt.bcf_bgzf;
    std::string header_text;
    {
        VcfReader hdr(o.vcf_path, "-");
        if (!hdr.ok()) {
            std::cerr << hdr.error << std::endl;
            return 1;
        }
        header_text = cleaned_header(hdr.header_lines, o.verbose); // main.cpp:505-510
    }
    if (!vcf_first->ok()) {
        std::cerr << vcf_first->error << std::endl;
        return 1;
    }
    if (!o.cohort) {
        std::cout << header_text;
        std::cout.flush();
    }
    pelapsed("VCF parsing and genotyping");

    // One pass over the panel (host/call_worker.hpp): the record loop here cuts the blocks and closes the batches, the pass takes them from there
    auto vcf_pass = [&](VcfReader &vcf, const uint32_t planes, PassOut &to) -> size_t {
        const bool iso_path = getenv("MALVA_GENO_ISO_PATH") && atoi(getenv("MALVA_GENO_ISO_PATH")) != 0;
        const BatchRules rules{o.k, o.haploid, vcf.keep.size() <= SPARSE_GT_SAMPLES && !vcf.defer_genotypes, vcf.keep.size(), iso_path, getenv("MALVA_GENO_HOST_ENUM") != nullptr,
                               want_sample, geno_batch_records(200000)};
        PanelPass pass(devs, o, planes, to, vcf.keep.size(), merged_fmt, priors_file, times);
        BatchBuilder<std::reference_wrapper<PanelPass>> batches(rules, contig_base, std::ref(pass)); // (which records a batch keeps, when it closes: host/panel_batch.hpp)
        const size_t n = for_each_block(vcf, o, refs, false, nullptr, std::ref(batches), &devs[0]);
        batches.flush();
        pass.finish();
        return n;
    };

    size_t n = 0;
    if (!o.cohort) {
        PassOut to;
        to.per_sample.emplace_back();
        to.per_sample[0].open("-", PartFile::STDOUT);
        n = vcf_pass(*vcf_first, 0, to);
    } else {
        Device &dev = devs[0];
        // --merged: a cohort that runs as ONE group writes its lines straight to the output (PATH.part, renamed at the end; stdout as it is).
        // Otherwise every group writes its block to a scratch file -- the first the header and whole lines, the others their sample columns
        // alone -- beside the output, or under $TMPDIR when that is stdout, and with --site-tags its records' counts to another (PATH.gN.cnt.part);
        // a last pass pastes them (host/cohort_out.hpp).  Whatever is left of these files goes when this frame is left, on success and on error.
        std::deque<PartFile> merged_blocks, merged_counts; // the first group's first
        PartFile merged_file;
        // --pairs: the table of the whole cohort, [samples][samples][9], of which the entries i < j are filled: a group's own pairs when its panel
        // pass ends, the pairs across two groups by the pass behind the last group, from the groups' packed words (PATH.gN.pack.part: 3 bits per cell)
        std::deque<PartFile> pack_files;
        const bool want_pairs = !o.pairs.empty();
        const size_t S = samples.size();
        std::vector<uint64_t> pair_table(want_pairs ? S * S * 9 : 0, 0);
        std::vector<size_t> group_first; // the first sample of every group
        // --sample-stats: [samples][MG_SAMPLE_SLOTS]; a sample belongs to one group, whose panel pass sums its row, so the table needs no pass of its own
        std::vector<uint64_t> sample_table(want_sample ? S * MG_SAMPLE_SLOTS : 0, 0);
        // --site-stats: a cohort that runs as ONE group writes the table's lines as its batches leave (PATH.part, renamed at the end).  Otherwise every
        // group leaves its records' counts in PATH.gN.geno.part, and the pass behind the last group sums them, tests the sums and writes the table
        const bool want_site = !o.site_stats.empty();
        std::deque<PartFile> geno_files;
        PartFile site_file;
        // --ld, --ibd, --grm: every group -- one group too -- leaves its records' words over its planes in PATH.gN.sites.part, one stream for the three,
        // beside the first of the three outputs that is given.  Their passes behind the last group read it one after the other, each with a reader of
        // its own.  --ld: r2 formed over all groups on the device.  --ibd: every pair of samples walked along the records on the device, chunk by chunk.
        // --grm: the chunks handed to the device, where the pairs' sums stay.  Each writes its table as PATH.part (--grm-format gcta: GCTA's three files).
        // The groups' streams go before a table takes its name: the tables are renamed behind the last of the passes, LD, IBD, GRM, so a failure in a
        // later pass leaves no earlier table under its name and no scratch file behind.
        const bool want_ld = !o.ld.empty(), want_ibd = !o.ibd.empty(), want_grm = !o.grm.empty();
        const std::string &site_words_base = want_ld ? o.ld : want_ibd ? o.ibd : o.grm;
        std::deque<PartFile> site_word_files;
        std::vector<size_t> site_word_group_sizes;
        PartFile ld_file, ibd_file, grm_file, grm_bin, grm_n_bin, grm_id;
        std::vector<std::string> names;
        for (const auto &sm : samples) names.push_back(sm.name);
        const bool merged_stdout = o.merged == "-";
        const std::string merged_tmp_base = !merged_stdout ? o.merged : std::string(getenv("TMPDIR") && *getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp") + "/malva-geno." + std::to_string((long)getpid()) + ".merged";
        auto open_merged = [&]() -> PartFile & { // (a failure names the file that could not be made)
            try {
                merged_file.open(o.merged, merged_stdout ? PartFile::STDOUT : PartFile::RENAMED);
            } catch (const std::runtime_error &) {
                throw std::runtime_error("cannot write " + o.merged + ".part");
            }
            return merged_file;
        };
        auto open_scratch = [](std::deque<PartFile> &files, const std::string &base, const char *ext) -> PartFile & { // the next group's BASE.gN<ext>
            files.emplace_back();
            files.back().open(base + ".g" + std::to_string(files.size() - 1) + ext, PartFile::SCRATCH);
            return files.back();
        };
        std::string merged_head;
        if (!o.merged.empty()) {
            VcfReader hdr(o.vcf_path, "-");
            if (!hdr.ok()) throw std::runtime_error(hdr.error);
            if (bcf_out) { // the text header with a ##contig line per reference sequence where the panel's header has none
                const bool declared = bcf_has_contig_lines(hdr.header_lines);
                merged_fmt.bcf_hdr = bcf_parse_header(merged_header(hdr.header_lines, o.verbose, names, o.site_tags,
                                                         declared ? std::vector<std::string>() : bcf_contig_lines(refs.names, refs.seqs), o.gp, o.pl),
                                           declared);
                merged_fmt.bcf_samples = samples.size();
                const std::string head = merged_fmt.bcf_hdr.file_head();
                if (bcf_bgzf) bgzf_append(head.data(), head.size(), merged_head);
                else merged_head = head;
            } else
                merged_head = merged_header(hdr.header_lines, o.verbose, names, o.site_tags, {}, o.gp, o.pl);
        }
        bool merged_direct = false; // one group: no temporary blocks
        std::vector<uint32_t> group_planes; // the samples of every group, in the order they ran
        size_t G = o.cohort_group ? (size_t)o.cohort_group : std::min<size_t>(samples.size(), 64);
        // --cohort-priors --prior-groups with a cohort in several groups: every group runs twice.  Its COVERAGE pass holds the samples' counters
        // and leaves the batches' coverages in BASE.gN.cov.part; the estimate pass behind the last group makes BASE.freq.part from all of them
        // (host/cohort_priors.hpp); its OUTPUT pass reads both, needs no counters and makes what a WHOLE group makes.  BASE: the merged output's
        // scratch base, else a name inside -o's directory.
        enum GroupPass { WHOLE, COVERAGE, OUTPUT };
        std::deque<PartFile> prior_cov_files;
        PartFile prior_freq_file;
        const std::string prior_base = !o.merged.empty() ? merged_tmp_base : o.out_dir + "/malva-geno.priors";
        bool prior_split = false;
        auto run_group = [&](const size_t s0, const GroupPass pass) -> size_t { // -> the group's samples
            size_t g = pass == OUTPUT ? group_planes[group_first.size()] : std::min(G, samples.size() - s0);
            if (pass != OUTPUT) {
                Timed t("cohort: planes");
                int rc = mg_cohort_begin(dev.ctx, (uint32_t)g);
                if (rc == MG_ERR_NOMEM && o.priors.on && !o.priors.groups && g > 1) throw std::runtime_error(prior_memory_error(samples.size())); // (no smaller groups: nothing has been written)
                while (rc == MG_ERR_NOMEM && !o.cohort_group && g > 1) { // (as many as fit beside the index)
                    G = g = (g + 1) / 2;
                    rc = mg_cohort_begin(dev.ctx, (uint32_t)g);
                }
                dev.check(rc, "mg_cohort_begin");
            }
            if (!o.out_dir.empty() && mkdir(o.out_dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("cannot create " + o.out_dir);
            GroupPass mode = pass;
            if (pass == WHOLE && s0 == 0 && o.priors.on && o.priors.groups && g < samples.size()) mode = COVERAGE, prior_split = true;
            else if (pass == WHOLE && prior_split) mode = COVERAGE;
            PassOut to; // (a group's files are written as NAME.vcf.part: a failure on the way leaves no truncated NAME.vcf behind)
            if (mode == COVERAGE) { // (nothing of the outputs exists yet)
                group_planes.push_back((uint32_t)g);
                {
                    Timed t("cohort: table scans");
                    for (size_t i = 0; i < g; ++i) {
                        dev.check(mg_cohort_select(dev.ctx, (uint32_t)i), "mg_cohort_select");
                        scan_sample(samples[s0 + i].input);
                    }
                }
                to.prior_cov = &open_scratch(prior_cov_files, prior_base, ".cov.part");
                to.prior_cov_panel = s0 == 0;
                {
                    Timed t("cohort: coverage pass");
                    std::unique_ptr<VcfReader> again;
                    if (s0) {
                        again.reset(new VcfReader(o.vcf_path, o.samples));
                        start_vcf(*again);
                        if (!again->ok()) throw std::runtime_error(again->error);
                    }
                    n = vcf_pass(s0 ? *again : *vcf_first, (uint32_t)g, to);
                }
                to.prior_cov->close("cannot write the coverages for the cohort's priors");
                dev.check(mg_cohort_end(dev.ctx), "mg_cohort_end");
                return g;
            }
            if (o.priors.on && !o.priors.out.empty() && s0 == 0) priors_file.open(o.priors.out); // (the first group writes the table: every group has the cohort's values)
            if (mode == WHOLE) group_planes.push_back((uint32_t)g);
            group_first.push_back(s0);
            PriorGroupInput prior_in;
            if (mode == OUTPUT) {
                prior_in.open(prior_cov_files[group_first.size() - 1].path, prior_freq_file.path, g);
                to.prior_in = &prior_in;
            }
            PairsRun pairs_run;
            if (want_pairs) {
                pairs_run.counts.assign(g * g * 9, 0);
                if (g != S) pairs_run.pack_out = &open_scratch(pack_files, o.pairs, ".pack.part"); // (several groups: their pairs across need every group's calls again)
            }
            if (mode == WHOLE) {
                Timed t("cohort: table scans");
                for (size_t i = 0; i < g; ++i) {
                    dev.check(mg_cohort_select(dev.ctx, (uint32_t)i), "mg_cohort_select");
                    scan_sample(samples[s0 + i].input);
                }
            }
            to.merged_fixed = s0 == 0;
            to.pairs = want_pairs ? &pairs_run : nullptr;
            to.sample_table = want_sample ? &sample_table[s0 * MG_SAMPLE_SLOTS] : nullptr;
            if (want_site) {
                to.site_stats_stream = g != S, to.site_stats_cols = s0 == 0, to.site_stats_samples = S;
                if (g != S) to.site_stats = &open_scratch(geno_files, o.site_stats, ".geno.part");
                else {
                    site_file.open(o.site_stats);
                    site_file.write(site_stats_header());
                    to.site_stats = &site_file;
                }
            }
            if (want_ld || want_ibd || want_grm) {
                to.site_words = &open_scratch(site_word_files, site_words_base, ".sites.part"), to.site_words_cols = s0 == 0;
                site_word_group_sizes.push_back(g);
                to.site_words_for = want_ld ? PassOut::LD : want_ibd ? PassOut::IBD : PassOut::GRM;
            }
            for (size_t i = 0; i < g && !o.out_dir.empty(); ++i) {
                to.per_sample.emplace_back();
                to.per_sample.back().open(o.out_dir + "/" + samples[s0 + i].name + ".vcf");
                to.per_sample.back().write(header_text);
            }
            if (!o.merged.empty()) {
                if (s0 == 0) merged_fmt.bcf_direct = merged_direct = g == samples.size();
                to.merged = merged_direct ? &open_merged() : &open_scratch(merged_blocks, merged_tmp_base, bcf_out ? ".bcf.part" : ".part");
                if (o.site_tags && !merged_direct) to.site_counts = &open_scratch(merged_counts, merged_tmp_base, ".cnt.part");
                // (BCF in several groups: the header goes in front of the pasted records, the groups' files hold records alone)
                if (s0 == 0 && (!bcf_out || merged_direct)) to.merged->write(merged_head, "cannot write the merged output");
            }
            {
                Timed t(mode == OUTPUT ? "cohort: output pass" : "cohort: panel pass");
                std::unique_ptr<VcfReader> again;
                if (s0 || mode == OUTPUT) { // (the panel does not stay resident across groups: it is read again)
                    again.reset(new VcfReader(o.vcf_path, o.samples));
                    start_vcf(*again);
                    if (!again->ok()) throw std::runtime_error(again->error);
                }
                n = vcf_pass(again ? *again : *vcf_first, (uint32_t)g, to);
            }
            priors_file.close(); // (a later group adds nothing; the table takes its name at the end)
            if (pairs_run.pack_out) pairs_run.pack_out->close("cannot write the pair table's packed calls");
            for (size_t i = 0; want_pairs && i < g; ++i)
                for (size_t j = i + 1; j < g; ++j) std::copy_n(&pairs_run.counts[(i * g + j) * 9], 9, &pair_table[((s0 + i) * S + s0 + j) * 9]);
            if (to.site_counts) to.site_counts->close("cannot write the merged output's counts");
            if (to.site_stats) to.site_stats->close(to.site_stats_stream ? "cannot write the per-record table's counts" : "cannot write the per-record table");
            if (to.site_words) to.site_words->close("cannot write the records' site words");
            if (to.merged) {
                if (bcf_out && bcf_bgzf && merged_direct) to.merged->write(bgzf_eof(), "cannot write the merged output");
                to.merged->close("cannot write the merged output");
            }
            // the group's files take their names when the group is complete, and only after every one of them is closed
            for (PartFile &f : to.per_sample) f.close("cannot write the output");
            for (PartFile &f : to.per_sample) f.finish();
            if (mode == WHOLE) dev.check(mg_cohort_end(dev.ctx), "mg_cohort_end");
            return g;
        }; // run_group
        for (size_t s0 = 0; s0 < samples.size();) s0 += run_group(s0, WHOLE);
        if (prior_split) {
            {
                Timed t("cohort: estimate pass");
                std::vector<std::string> paths;
                for (const PartFile &f : prior_cov_files) paths.push_back(f.path);
                prior_freq_file.open(prior_base + ".freq.part", PartFile::SCRATCH);
                walk_prior_groups(paths, group_planes, prior_range_bytes(),
                                  [&](size_t nr, size_t planes, const uint32_t *cov, const float *f0, const uint32_t *var_allele_off, float *f_t, uint32_t *n_inf) {
                                      dev.check(mg_estimate_priors(dev.ctx, nr, (uint32_t)planes, cov, f0, var_allele_off, o.error_rate, (int)o.max_coverage, o.haploid,
                                                                   o.priors.iters, o.priors.weight, f_t, n_inf),
                                                "mg_estimate_priors");
                                      float ms = 0;
                                      dev.check(mg_estimate_priors_stats(dev.ctx, &ms), "mg_estimate_priors_stats");
                                      times.estimate.add(&ms, 1);
                                  },
                                  [&](const std::string &bytes) { prior_freq_file.write(bytes, "cannot write the cohort's priors"); });
                prior_freq_file.close("cannot write the cohort's priors");
            }
            for (size_t s0 = 0; s0 < samples.size();) s0 += run_group(s0, OUTPUT);
        }
        if (!o.merged.empty() && !merged_direct) { // the groups' blocks pasted record by record (host/cohort_out.hpp)
            Timed t("cohort: merged paste");
            SiteCountsReader counts(merged_counts);
            GroupFiles in;
            in.open(merged_blocks);
            open_merged();
            auto sink = [&](const char *data, size_t n) { merged_file.write(data, n, "cannot write the merged output"); };
            if (bcf_out) {
                sink(merged_head.data(), merged_head.size());
                paste_bcf_groups(in.f, group_planes, merged_fmt.n_fields(o), (uint32_t)merged_fmt.bcf_samples, merged_fmt.bcf_hdr, o.site_tags ? &counts : nullptr, bcf_bgzf, sink);
            } else {
                // --site-tags: the groups' counts summed, 65,536 records at a time (MALVA_GENO_BATCH, when set: tests), and their INFO strings made on the device
                const size_t paste_batch = geno_batch_records(65536);
                std::vector<uint32_t> p_ac, p_ns, p_vao;
                paste_text_groups(in.f, o.site_tags, [&](std::vector<char> &text, std::vector<uint64_t> &off) {
                    counts.next_batch(paste_batch, p_ac, p_ns, p_vao);
                    site_info(dev, p_ns.size(), p_ac.data(), p_ns.data(), p_vao.data(), text, off, times);
                }, sink);
            }
            merged_file.close("cannot write the merged output");
        }
        if (!o.merged.empty()) merged_file.finish();
        if (want_pairs) {
            Timed t("cohort: pair pass");
            std::vector<uint64_t> cross; // the pairs across two groups, from the groups' packed words
            for (size_t gi = 0; gi < pack_files.size(); ++gi)
                for (size_t gj = gi + 1; gj < pack_files.size(); ++gj) {
                    const size_t ga = group_planes[gi], gb = group_planes[gj];
                    cross.assign(ga * gb * 9, 0);
                    walk_pack_pair(pack_files[gi].path, ga, pack_files[gj].path, gb, [&](size_t W, const uint64_t *words_a, const uint64_t *words_b) {
                        dev.check(mg_pair_counts(dev.ctx, W, words_a, (uint32_t)ga, words_b, (uint32_t)gb, 1, cross.data()), "mg_pair_counts");
                        float ms[2] = {0, 0};
                        dev.check(mg_pairs_stats(dev.ctx, ms), "mg_pairs_stats");
                        times.pairs.ms[1] += ms[1];
                        ++times.pairs.calls[1];
                    });
                    for (size_t i = 0; i < ga; ++i)
                        std::copy_n(&cross[i * gb * 9], gb * 9, &pair_table[((group_first[gi] + i) * S + group_first[gj]) * 9]);
                }
            PartFile::put(o.pairs, pair_table_text(names, pair_table.data()));
        }
        if (want_sample) PartFile::put(o.sample_stats, sample_table_text(names, sample_table.data()));
        if (want_site && !geno_files.empty()) {
            Timed t("cohort: site table pass");
            site_file.open(o.site_stats);
            site_stats_groups(
                geno_files, S, o.haploid, geno_batch_records(65536),
                [&](size_t n_items, const uint32_t *n, const uint32_t *het, const uint32_t *hom, double *hwe, double *exc) {
                    dev.check(mg_hwe_exact(dev.ctx, n_items, n, het, hom, hwe, exc), "mg_hwe_exact");
                    float ms[2] = {0, 0};
                    dev.check(mg_hwe_stats(dev.ctx, ms), "mg_hwe_stats");
                    times.geno.ms[1] += ms[1];
                    ++times.geno.calls[1];
                },
                [&](const char *data, size_t n) { site_file.write(data, n, "cannot write the per-record table"); });
            geno_files.clear(); // (the groups' streams go before the table takes its name)
        }
        if (want_site) site_file.finish("cannot write the per-record table");
        if (want_ld) {
            Timed t("cohort: ld pass");
            ld_file.open(o.ld);
            ld_table(
                site_word_files, o.ld_window, geno_batch_records(65536),
                [&](size_t n_vars, size_t n_first, size_t n_groups, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, mg_ld_pair *pairs, size_t cap,
                    uint64_t *row_off, uint64_t *needed) {
                    const int rc = mg_ld_window(dev.ctx, n_vars, n_first, (uint32_t)n_groups, sites, chrom, pos, o.ld_window, o.ld_window_bp, o.ld_min_n, o.ld_min_r2, pairs, cap,
                                                row_off, needed);
                    if (rc != MG_ERR_LIMIT) dev.check(rc, "mg_ld_window");
                    float ms[2] = {0, 0};
                    dev.check(mg_ld_stats(dev.ctx, ms), "mg_ld_stats");
                    times.ld.ms[1] += ms[1];
                    ++times.ld.calls[1];
                    return rc;
                },
                [&](const char *data, size_t n) { ld_file.write(data, n, "cannot write the LD table"); });
            ld_file.close("cannot write the LD table");
        }
        if (want_ibd) {
            Timed t("cohort: ibd pass");
            ibd_file.open(o.ibd);
            if (S >= 2) dev.check(mg_ibd_begin(dev.ctx, (uint32_t)S, o.ibd_min_records, o.ibd_min_bp), "mg_ibd_begin");
            ibd_table(
                site_word_files, site_word_group_sizes, names, geno_batch_records(65536),
                [&](size_t n_vars, size_t n_groups, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, int flush, mg_ibd_seg *segs, size_t cap, uint64_t *needed) {
                    const int rc = mg_ibd_step(dev.ctx, n_vars, (uint32_t)n_groups, sites, chrom, pos, flush, segs, cap, needed);
                    if (rc != MG_ERR_LIMIT) dev.check(rc, "mg_ibd_step");
                    float ms[2] = {0, 0};
                    dev.check(mg_ibd_stats(dev.ctx, ms), "mg_ibd_stats");
                    times.ibd.ms[1] += ms[1];
                    ++times.ibd.calls[1];
                    return rc;
                },
                [&](const char *data, size_t n) { ibd_file.write(data, n, "cannot write the IBD table"); });
            if (S >= 2) dev.check(mg_ibd_end(dev.ctx), "mg_ibd_end");
            ibd_file.close("cannot write the IBD table");
        }
        if (want_grm) {
            Timed t("cohort: grm pass");
            if (o.grm_gcta) grm_bin.open(o.grm + ".grm.bin"), grm_n_bin.open(o.grm + ".grm.N.bin"), grm_id.open(o.grm + ".grm.id");
            else grm_file.open(o.grm);
            dev.check(mg_grm_begin(dev.ctx, (uint32_t)S, o.haploid, o.grm_maf_ppm, o.grm_min_n), "mg_grm_begin");
            const GrmState st = grm_table(
                site_word_files, site_word_group_sizes, geno_batch_records(65536),
                [&](size_t n_vars, size_t n_groups, const uint64_t *sites) {
                    dev.check(mg_grm_step(dev.ctx, n_vars, (uint32_t)n_groups, sites), "mg_grm_step");
                    float ms[3] = {0, 0, 0};
                    dev.check(mg_grm_stats(dev.ctx, ms), "mg_grm_stats");
                    times.grm.ms[1] += ms[0], times.grm.ms[2] += ms[1];
                    ++times.grm.calls[1];
                },
                [&](int64_t *sum, uint64_t *count, uint64_t *records) { dev.check(mg_grm_read(dev.ctx, sum, count, records), "mg_grm_read"); });
            dev.check(mg_grm_end(dev.ctx), "mg_grm_end");
            std::cerr << "[malva-geno] grm: " << st.records[0] << " records seen, " << st.records[1] << " entered" << std::endl;
            const char *what = "cannot write the GRM";
            if (o.grm_gcta)
                grm_gcta(
                    st, names, [&](const char *data, size_t n) { grm_bin.write(data, n, what); }, [&](const char *data, size_t n) { grm_n_bin.write(data, n, what); },
                    [&](const char *data, size_t n) { grm_id.write(data, n, what); });
            else grm_text(st, names, [&](const char *data, size_t n) { grm_file.write(data, n, what); });
            for (PartFile *f : {&grm_file, &grm_bin, &grm_n_bin, &grm_id}) f->close(what);
        }
        site_word_files.clear(); // (the groups' streams go before a table takes its name)
        for (PartFile *f : {&ld_file, &ibd_file, &grm_file, &grm_bin, &grm_n_bin, &grm_id}) f->finish(); // (closed above; one that was never opened takes no name)
        priors_file.finish();
        times.add_to_timers();
        std::cerr << times.report();
    }
    if (times.gt_bytes) std::cerr << "[malva-geno] panel genotypes of the general blocks: " << times.gt_bytes << " bytes uploaded" << std::endl;
    pelapsed("Processed " + std::to_string(n) + " variants");
    pelapsed("Execution completed");
    return 0;
}

// index-convert: rewrite the index of <variants.vcf> in the other container (third argument: zst | hipz); host only
int convert_main(const Options &o)
{
    IndexPayload p;
    const bool to_zst = o.kmc_path == "zst";
    if (!to_zst && o.kmc_path != "hipz") throw std::runtime_error("index-convert: the third argument names the target container, zst or hipz");
    if (to_zst) {
        load_index_hipz(index_path(o, ".hipz"), p, o.k, o.ref_k, o.bf_size, STRIDE);
        save_index_zst(index_path(o, ".zst"), p, o.bf_size);
    } else {
        load_index_zst(index_path(o, ".zst"), p, o.bf_size, STRIDE);
        save_index_hipz(index_path(o, ".hipz"), p, o.k, o.ref_k, o.bf_size);
    }
    std::cerr << "[malva-geno] index rewritten as " << index_path(o, to_zst ? ".zst" : ".hipz") << ": " << p.filt[0].pos.size() << " + " << p.filt[1].pos.size()
              << " filter bits, " << p.vals.size() << " keys" << std::endl;
    return 0;
}

// dump-kmers: host-only view of the enumerator (tests compare it with the oracle's block model)
int dump_main(const Options &o)
{
    Reference refs;
    if (!read_fasta(o.fasta_path, o.strip_chr, refs)) {
        std::cerr << "ERROR: cannot open " << o.fasta_path << std::endl;
        return 1;
    }
    VcfReader vcf(o.vcf_path, o.samples);
    if (!vcf.ok()) {
        std::cerr << vcf.error << std::endl;
        return 1;
    }
    const bool for_index = o.kmc_path == "index";
    for_each_block(vcf, o, refs, for_index, nullptr, [&](Block &vb, const std::string &, const std::string &reference) {
        const auto sigs = vb.signatures(reference, o.haploid);
        std::cout << "BLOCK " << vb.vars.size() << (vb.is_lone_short() ? " lone" : "") << "\n";
        for (size_t vi = 0; vi < vb.vars.size(); ++vi) {
            const Variant &v = vb.vars[vi];
            std::cout << "VAR " << v.seq_name << " " << v.ref_pos + 1 << " " << v.ref_sub;
            for (const auto &a : v.alts) std::cout << " " << a;
            std::cout << " present=" << v.is_present << "\n";
            for (const auto &as : sigs[vi]) {
                std::vector<std::string> lines;
                for (const auto &sig : as.second) {
                    std::string l;
                    for (const auto &kmer : sig) l += (l.empty() ? "" : ",") + kmer;
                    lines.push_back(l);
                }
                std::sort(lines.begin(), lines.end()); // signature order is unordered_set order in the reference
                for (const auto &l : lines) std::cout << "SIG " << as.first << " " << l << "\n";
            }
        }
    });
    return 0;
}

// ---- pca: the principal components of a GRM that `call --cohort --grm` wrote (pca.hpp; mg_pca_* in include/malva_hip.h) -----------------
// Its own parser and usage text; no index and no panel: the context is the smallest mg_create makes.
int pca_main(int argc, char **argv)
{
    PcaOptions o;
    const PcaParsed parsed = pca_parse(argc, argv, o, std::cerr);
    if (parsed == PcaParsed::help) std::cout << PCA_USAGE;
    if (parsed != PcaParsed::ok) return parsed == PcaParsed::help ? EXIT_SUCCESS : EXIT_FAILURE;
    try {
        PcaInput in;
        {
            Timed t("pca: read");
            in = pca_read(o.grm);
        }
        PcaResult r;
        r.n = (uint32_t)in.names.size();
        r.k = o.pcs;
        r.tol = o.tol;
        if (r.k > r.n) {
            std::cerr << "[malva-geno] --pcs " << o.pcs << " lowered to the " << r.n << " sample(s) of " << o.grm << std::endl;
            r.k = r.n;
        }
        Device dev;
        if (mg_create(&dev.ctx, o.device, 1, 1, 1) != MG_OK) throw std::runtime_error("no usable MI355X/HIP device " + std::to_string(o.device) + "; this build has no CPU path");
        {
            Timed t("pca: load");
            dev.check(in.packed ? mg_pca_load_tri_f32(dev.ctx, r.n, in.tri.data()) : mg_pca_load_f64(dev.ctx, r.n, in.full.data()), "mg_pca_load");
        }
        std::vector<float>().swap(in.tri);
        std::vector<double>().swap(in.full);
        r.values.resize(r.k), r.resid.resize(r.k), r.vectors.resize((size_t)r.k * r.n);
        {
            Timed t("pca: solve");
            dev.check(mg_pca_solve(dev.ctx, r.k, o.tol, o.max_iters, r.values.data(), r.vectors.data(), r.resid.data(), &r.scale, r.info), "mg_pca_solve");
        }
        dev.check(mg_pca_stats(dev.ctx, r.ms), "mg_pca_stats");
        dev.check(mg_pca_end(dev.ctx), "mg_pca_end");
        pca_write(o.out, r, in.names, in.trace);
        const uint32_t first = pca_first_unconverged(r);
        std::cerr << "[malva-geno] pca: " << r.k << " component(s) of " << r.n << " sample(s), " << r.info[0] << " product(s), block of " << r.info[2] << std::endl;
        if (first < r.k) {
            std::cerr << "malva : pca: component " << first + 1 << " is not converged after " << r.info[0] << " product(s) (residual " << r.resid[first] << ", --tol " << o.tol
                      << "); " << r.info[1] << " of " << r.k << " are" << std::endl;
            return 2;
        }
        return EXIT_SUCCESS;
    } catch (const std::exception &e) {
        std::cerr << "malva : " << e.what() << std::endl;
        return EXIT_FAILURE;
    }
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::cerr << "malva missing arguments\n" << USAGE << std::endl;
        return 1;
    }
    const std::string cmd = argv[1];
    if (cmd == "pca") return pca_main(argc - 1, argv + 1); // (before parse_arguments: OPTIONS and USAGE are index's and call's)
    int (*const run)(const Options &) = cmd == "index-convert"            ? convert_main
                                        : cmd.compare(0, 5, "index") == 0 ? index_main
                                        : cmd.compare(0, 4, "call") == 0  ? call_main
                                        : cmd == "dump-kmers"             ? dump_main
                                                                          : nullptr;
    if (!run) {
        std::cerr << "Could not interpret command " << argv[1] << ".\nAccepted commands are index and call." << std::endl;
        return 1;
    }
    try {
        Options o;
        const Parsed parsed = parse_arguments(argc - 1, argv + 1, o, std::cerr);
        if (parsed == Parsed::help) std::cout << USAGE;
        return parsed == Parsed::ok ? run(o) : parsed == Parsed::help ? EXIT_SUCCESS : EXIT_FAILURE;
    } catch (const std::exception &e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        return 1;
    }
}
