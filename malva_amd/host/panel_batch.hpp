// A batch of panel records, flattened for the device: the arrays of general blocks and of lone records, the panel's genotype words, and the rules
// by which `call` fills and closes its batches.  Host only: tools/call_batch_host_check.cpp drives all of it without a device (`make sanitize-host`).
#pragma once
#include "../../include/malva_hip.h" // (MG_MAX_KMER, MG_MAX_PACKED_K; nothing here calls the library)
#include "block.hpp"

namespace malva {

constexpr size_t STRIDE = 136; // MG_MAX_KMER + NUL, rounded to 8
// fixed-stride ASCII rows for the batch calls
struct Rows {
    std::vector<char> data;
    size_t n = 0;
    void add(const std::string &kmer)
    {
        if (kmer.empty() || kmer.size() > MG_MAX_KMER) throw std::runtime_error("signature k-mer of length " + std::to_string(kmer.size()) + " (1.." +
                                                                                std::to_string(MG_MAX_KMER) + " supported)");
        data.resize(data.size() + STRIDE, 0);
        memcpy(&data[n * STRIDE], kmer.data(), kmer.size());
        ++n;
    }
    void clear() { data.clear(), n = 0; }
};

// records per device round trip of `call`, and per batch of the merged paste; MALVA_GENO_BATCH exists so tests can force many small batches
inline size_t geno_batch_records(size_t dflt) { return getenv("MALVA_GENO_BATCH") ? (size_t)std::max(1L, atol(getenv("MALVA_GENO_BATCH"))) : dflt; }

// the concatenated reference the device holds (mg_reference_upload); contig_base: where every sequence starts in it
inline std::string concat_reference(const Reference &refs, std::map<std::string, uint64_t> &contig_base)
{
    std::string all;
    for (const auto &name : refs.names) {
        contig_base[name] = all.size();
        all += refs.seqs.at(name);
    }
    return all;
}

// build_alleles_combs on a chain of one (var_block.hpp:734-786): the (canonical) alleles some kept haplotype carries
inline uint64_t carried_mask(const Variant &v, bool haploid)
{
    uint64_t mask = 0;
    if (v.gt_deferred) {
        if (v.max_allele >= (uint32_t)v.n_alleles()) (void)v.alts.at(v.max_allele); // (throws what the loop below would)
        for (int a = 0; a < v.n_alleles() && a < 64; ++a)
            if ((v.raw_mask >> a) & 1) mask |= 1ULL << v.allele_index(v.allele(a));
        return mask;
    }
    for (size_t g = 0; g < v.genotypes.size(); ++g) {
        mask |= 1ULL << v.allele_index(v.allele(v.genotypes[g].first));
        if (!haploid) mask |= 1ULL << v.allele_index(v.allele(v.genotypes[g].second));
    }
    return mask;
}

// The panel genotypes of a batch of blocks, as the device takes them.  Dense: one [variant][sample] matrix of a1 | a2 << 7 | phased << 14.  Sparse
// (panels of more than SPARSE_GT_SAMPLES samples, nearly all 0|0): per variant only the samples that carry anything else, in sample order
constexpr uint32_t SPARSE_GT_SAMPLES = 64;
struct PanelGenotypes {
    bool sparse = false;
    std::vector<uint16_t> gt;                 // dense
    std::vector<uint32_t> sp_off{0}, sp_sample; // sparse
    std::vector<uint16_t> sp_gt;
    uint16_t sp_default = (uint16_t)(1u << 14);
    size_t bytes() const { return sparse ? 4 * sp_off.size() + 6 * sp_sample.size() : 2 * gt.size(); }
};
// one sample's genotype as the device takes it: a1 | a2 << 7 | phased << 14
inline uint16_t genotype_word(const Variant &v, size_t s_, bool haploid)
{
    const auto &p2 = v.genotypes[s_];
    if (p2.first >= v.n_alleles() || p2.second >= v.n_alleles())
        throw std::runtime_error("GT allele beyond the kept ALT list at " + v.seq_name + ":" + std::to_string(v.ref_pos + 1) +
                                 " (the reference reads out of bounds here)");
    if (haploid) return (uint16_t)(p2.first | (1u << 14));
    return (uint16_t)(p2.first | (p2.second << 7) | ((v.phasing[s_] ? 1 : 0) << 14));
}
inline PanelGenotypes pack_genotypes(const std::vector<const Variant *> &vars, size_t n_vars, uint32_t n_samples, bool haploid)
{
    PanelGenotypes g;
    g.sparse = n_samples > SPARSE_GT_SAMPLES;
    for (const Variant *vp : vars) g.sparse = g.sparse || vp->gt_deferred; // (records decoded on the device arrive in the sparse form whatever the panel's size)
    if (!g.sparse) g.gt.assign(n_vars * n_samples, 0);
    // haploid mode reads the first allele only (var_block.hpp:751): the word is reduced to it, so that a ploidy-1 panel is as sparse as it looks
    auto word = [&](const Variant &v, size_t s_) -> uint16_t { return genotype_word(v, s_, haploid); };
    if (g.sparse) { // the default word: 0|0 phased or 0/0 unphased, whichever the batch holds more of (a sample of it decides)
        size_t phased0 = 0, unphased0 = 0, seen = 0;
        for (const Variant *vp : vars) {
            const Variant &v = *vp;
            if (v.gt_deferred) { // decoded on the device: its batch's default stands for its samples
                (v.sp_default ? phased0 : unphased0) += 64;
                seen += 64;
            } else
                for (size_t s_ = 0; s_ < v.genotypes.size() && seen < 200000; s_ += 7, ++seen) {
                    const uint16_t w = word(v, s_);
                    phased0 += w == (1u << 14);
                    unphased0 += w == 0;
                }
            if (seen >= 200000) break;
        }
        g.sp_default = unphased0 > phased0 ? 0 : (uint16_t)(1u << 14);
    }
    size_t row = 0;
    for (const Variant *vp : vars) {
            const Variant &v = *vp;
            if (v.gt_deferred) { // already the sparse layout (mg_decode_gt_text), against its own batch's default
                if (!g.sparse) throw std::runtime_error("internal: deferred genotypes on a panel of few samples");
                if (v.max_allele >= (uint32_t)v.n_alleles())
                    throw std::runtime_error("GT allele beyond the kept ALT list at " + v.seq_name + ":" + std::to_string(v.ref_pos + 1) +
                                             " (the reference reads out of bounds here)");
                if (v.sp_default == g.sp_default) {
                    g.sp_sample.insert(g.sp_sample.end(), v.sp_sample.begin(), v.sp_sample.end());
                    g.sp_gt.insert(g.sp_gt.end(), v.sp_gt.begin(), v.sp_gt.end());
                } else { // (a panel that mixes phased and unphased records: the samples WITHOUT an entry are the ones that differ here)
                    size_t e = 0;
                    for (uint32_t s_ = 0; s_ < v.n_kept; ++s_) {
                        uint16_t w = v.sp_default;
                        if (e < v.sp_sample.size() && v.sp_sample[e] == s_) w = v.sp_gt[e++];
                        if (w != g.sp_default) {
                            g.sp_sample.push_back(s_);
                            g.sp_gt.push_back(w);
                        }
                    }
                }
                g.sp_off.push_back((uint32_t)g.sp_sample.size());
                ++row;
                continue;
            }
            for (size_t s_ = 0; s_ < v.genotypes.size(); ++s_) {
                const uint16_t w = word(v, s_);
                if (!g.sparse) g.gt[row * n_samples + s_] = w;
                else if (w != g.sp_default) {
                    g.sp_sample.push_back((uint32_t)s_);
                    g.sp_gt.push_back(w);
                }
            }
            if (g.sparse) g.sp_off.push_back((uint32_t)g.sp_sample.size());
            ++row;
        }
    return g;
}

inline PanelGenotypes pack_genotypes(const std::vector<Block> &blocks, size_t n_vars, uint32_t n_samples, bool haploid)
{
    std::vector<const Variant *> vars;
    vars.reserve(n_vars);
    for (const Block &b : blocks)
        for (const Variant &v : b.vars) vars.push_back(&v);
    return pack_genotypes(vars, n_vars, n_samples, haploid);
}
inline PanelGenotypes pack_genotypes(const std::vector<Variant> &records, size_t n_vars, uint32_t n_samples, bool haploid)
{
    std::vector<const Variant *> vars;
    vars.reserve(records.size());
    for (const Variant &v : records) vars.push_back(&v);
    return pack_genotypes(vars, n_vars, n_samples, haploid);
}

// the lone-record kernels read ceil(k/2) bases right of the REF allele: true when the contig holds them (else the k-mer is clipped, var_block.hpp:187)
inline bool right_flank_fits(const Variant &v, unsigned k, size_t ref_len) { return (long)v.ref_pos + v.ref_size + (long)(k + 1) / 2 <= (long)ref_len; }

struct LoneArrays { // inputs of mg_index_isolated and mg_call_isolated: blocks of one record, every allele shorter than k
    std::vector<uint64_t> pos, present;
    std::vector<uint32_t> var_allele_off{0}, allele_off{0};
    std::vector<char> pool;
    std::vector<uint8_t> flags;
    size_t n() const { return var_allele_off.size() - 1; }
    template <class F> [[gnu::always_inline]] void add_alleles(const Variant &v, F per_allele) // the record's alleles end to end (inlined: once per record on the parsing thread)
    {
        const uint32_t A = (uint32_t)v.n_alleles();
        for (uint32_t a = 0; a < A; ++a) {
            const std::string &al = v.allele((int)a);
            pool.insert(pool.end(), al.begin(), al.end());
            allele_off.push_back((uint32_t)pool.size());
            per_allele(al);
        }
        var_allele_off.push_back(var_allele_off.back() + A);
    }
    [[gnu::always_inline]] void add(const Variant &v, uint64_t base, unsigned k, size_t ref_len, bool haploid)
    {
        const bool eligible = v.is_present && v.ref_pos >= (int)k && v.ref_pos <= (int)ref_len - (int)k; // var_block.hpp:104
        pos.push_back(base + (uint64_t)std::max(v.ref_pos, 0));
        present.push_back(eligible ? carried_mask(v, haploid) : 0);
        flags.push_back(eligible ? 1 : 0);
        add_alleles(v, [](const std::string &) {});
    }
};
struct BlockArrays : LoneArrays { // inputs of mg_index_blocks / mg_cover_blocks*: the base's three allele arrays (its other three stay empty) and eight more
    std::vector<uint64_t> blk_base;
    std::vector<uint32_t> blk_len, blk_var_off{0}, ref_size, min_size;
    std::vector<int32_t> ipos;
    std::vector<uint8_t> is_present, canon;
    bool wide_alleles = false; // a record of more than 127 alleles: the device's 7-bit allele numbers cannot hold it
    size_t n_blocks() const { return blk_base.size(); }
    void open_block(uint64_t base, size_t ref_len) { blk_base.push_back(base), blk_len.push_back((uint32_t)ref_len); }
    [[gnu::always_inline]] void add(const Variant &v)
    {
        if (v.n_alleles() > 127) wide_alleles = true;
        ipos.push_back(v.ref_pos); ref_size.push_back((uint32_t)v.ref_size); min_size.push_back((uint32_t)v.min_size); is_present.push_back(v.is_present);
        add_alleles(v, [&](const std::string &al) { canon.push_back((uint8_t)std::min(255, v.allele_index(al))); });
    }
    void close_block() { blk_var_off.push_back((uint32_t)n()); }
    // the batch as the library's host forms take it, with pg's dense or sparse half for the panel genotypes; points into both, owns nothing
    mg_blocks_host view(const PanelGenotypes &pg, uint32_t n_samples) const
    {
        mg_blocks_host x{};
        x.n_blocks = n_blocks(), x.blk_ref_base = blk_base.data(), x.blk_ref_len = blk_len.data(), x.blk_var_off = blk_var_off.data();
        x.n_vars = n(), x.pos = ipos.data(), x.ref_size = ref_size.data(), x.min_size = min_size.data(), x.present = is_present.data();
        x.var_allele_off = var_allele_off.data(), x.allele_off = allele_off.data(), x.pool = pool.data(), x.pool_len = pool.size(), x.canon = canon.data();
        x.n_samples = n_samples, x.sp_default = pg.sp_default;
        if (pg.sparse) x.sp_off = pg.sp_off.data(), x.sp_sample = pg.sp_sample.data(), x.sp_gt = pg.sp_gt.data();
        else x.gt = pg.gt.data();
        return x;
    }
};

// v.genotypes / v.phasing of a deferred record, for the host enumerator (a block the device handed back, dump-kmers' cousin paths)
inline void genotypes_from_entries(Variant &v)
{
    if (!v.gt_deferred) return;
    const auto pair_of = [](uint16_t w) { return std::make_pair((int)(w & 127), (int)((w >> 7) & 127)); };
    v.genotypes.assign(v.n_kept, pair_of(v.sp_default));
    v.phasing.assign(v.n_kept, (uint8_t)((v.sp_default >> 14) & 1));
    for (size_t e = 0; e < v.sp_sample.size(); ++e) {
        v.genotypes[v.sp_sample[e]] = pair_of(v.sp_gt[e]);
        v.phasing[v.sp_sample[e]] = (uint8_t)((v.sp_gt[e] >> 14) & 1);
    }
    v.gt_deferred = false;
    v.sp_sample.clear();
    v.sp_gt.clear();
}
inline void genotypes_from_entries(Block &b)
{
    for (Variant &v : b.vars) genotypes_from_entries(v);
}

struct SignatureRows { Rows rows; std::vector<uint8_t> is_ref; std::vector<uint64_t> sig_off{0}, al_off{0}; }; // what mg_lookup_cover takes
inline SignatureRows signature_rows(const Block &blk, const std::vector<AlleleSignatures> &sigs) // of a block the host enumerated (Block::extract)
{
    SignatureRows s;
    for (size_t vi = 0; vi < blk.vars.size(); ++vi)
        for (int a = 0; a < blk.vars[vi].n_alleles(); ++a) {
            auto it = sigs[vi].find(a);
            if (it != sigs[vi].end())
                for (const auto &sig : it->second) {
                    for (const auto &kmer : sig) {
                        s.rows.add(kmer);
                        s.is_ref.push_back(a == 0);
                    }
                    s.sig_off.push_back(s.rows.n);
                }
            s.al_off.push_back(s.sig_off.size() - 1);
        }
    return s;
}

// one output record waiting for its device results
struct Rec {
    std::string prefix; // CHROM .. QUAL columns
    uint32_t n_alleles;
    bool isolated;
    size_t slot;     // variant index inside its batch
    size_t allele0;  // first allele slot inside its batch
    size_t gt0;      // first genotype slot inside its batch
};
struct Batch : BlockArrays { // inputs of mg_call_isolated (the lone arrays) or mg_cover_blocks + mg_genotype (all eleven)
    std::vector<uint8_t> allele_class; // --sample-stats: one byte per allele slot (allele_class_of; slot 0 of a record: 0), else empty
    std::vector<float> freq;
    std::vector<uint64_t> var_gt_off{0};
    // general blocks: the records are kept until the batch has run, for the panel genotypes and for the blocks the device hands back
    std::vector<Variant> vars;
    std::vector<int32_t> var_slot;  // record -> its place in `vars`, or -1: a lone record the device cannot hand back, not kept
    std::vector<uint16_t> gt_dense; // a panel of few samples: the genotype words, made as the records are batched (else packed from `vars` by the worker)
    bool dense_gt = false;
    std::vector<const std::string *> block_ref;
    size_t genotype_cells = 0;
    // results
    std::vector<uint32_t> cov;
    std::vector<int32_t> g1, g2, gq;
    std::vector<uint8_t> status;
    std::vector<double> probs;
    std::vector<float> freq_out;   // --cohort-priors: the re-estimated frequencies, as freq
    std::vector<uint32_t> n_inf;   // --cohort-priors: per record, the planes that counted
    std::vector<int32_t> pl;       // --pl: [plane][genotype slot], a record's values in VCF order (mg_phred_likelihoods)
};

// --sample-stats: the kind of the ALT allele `alt` of a record whose REF is `ref`, from the strings as the record prints them (the class
// codes of mg_sample_counts: 1 transition, 2 transversion, 3 insertion, 4 deletion, 5 other)
inline uint8_t allele_class_of(const std::string &ref, const std::string &alt)
{
    if (alt == "*" || (!alt.empty() && alt[0] == '<')) return 5;
    auto base = [](char c) -> int {
        switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
        }
    };
    for (char c : alt)
        if (base(c) < 0) return 5;
    if (ref.size() == 1 && alt.size() == 1) return base(ref[0]) >= 0 && (base(ref[0]) ^ base(alt[0])) == 2 ? 1 : 2; // (A <-> G: 0 ^ 2, C <-> T: 1 ^ 3)
    if (alt.size() > ref.size()) return 3;
    if (alt.size() < ref.size()) return 4;
    return 5;
}

// What decides how `call` batches a panel.  dense_gt: few samples, all genotypes decoded on the host: the words are made while batching; iso_path,
// host_enum: MALVA_GENO_ISO_PATH, MALVA_GENO_HOST_ENUM; want_sample: --sample-stats; a batch closes at batch_records, or cell_bound genotype cells
struct BatchRules {
    unsigned k; bool haploid, dense_gt; size_t n_samples_kept;
    bool iso_path, host_enum, want_sample; size_t batch_records, cell_bound = 200u << 20;
};

// The blocks of one pass over the panel, batch by batch: close(recs, iso, gen) takes a batch (rvalues); the caller ends the pass with a flush()
template <class Close> struct BatchBuilder {
    const BatchRules r;
    const std::map<std::string, uint64_t> &contig_base;
    Close close;
    std::vector<Rec> recs;
    Batch iso, gen;
    std::string base_name; // (as for_each_block's ref_of: one map lookup per sequence, not per record)
    bool base_known = false;
    std::map<std::string, uint64_t>::const_iterator base_at;

    BatchBuilder(const BatchRules &rules, const std::map<std::string, uint64_t> &bases, Close c) : r(rules), contig_base(bases), close(std::move(c)) { fresh(); }
    void fresh()
    {
        recs.clear();
        iso = Batch(), gen = Batch(), gen.dense_gt = r.dense_gt;
        const size_t n = r.batch_records + 64; // (a batch's vectors at their final size at once: fifteen of them grew by doubling, record by record)
        Batch &b = gen;
        for (auto *v32 : {&b.blk_len, &b.blk_var_off, &b.ref_size, &b.min_size, &b.var_allele_off}) v32->reserve(n + 1);
        b.allele_off.reserve(2 * n + 1); b.blk_base.reserve(n); b.ipos.reserve(n); b.is_present.reserve(n); b.canon.reserve(2 * n); gen.freq.reserve(2 * n); b.pool.reserve(4 * n);
        gen.var_gt_off.reserve(n + 1); gen.var_slot.reserve(n); gen.block_ref.reserve(n);
        if (gen.dense_gt) gen.gt_dense.reserve(n * r.n_samples_kept);
    }
    void flush() { close(std::move(recs), std::move(iso), std::move(gen)), fresh(), recs.reserve(r.batch_records + 64); }
    void operator()(Block &vb, const std::string &seq_name, const std::string &reference) { add_block(vb, seq_name, reference); } // (what the record loop hands its blocks to)
    void add_block(Block &vb, const std::string &seq_name, const std::string &reference)
    {
        if (!base_known || seq_name != base_name) {
            base_at = contig_base.find(seq_name); base_name = seq_name; base_known = true;
        }
        const bool base_found = base_at != contig_base.end();
        const uint64_t base_value = base_found ? base_at->second : 0;
        auto add_rec = [&](Batch &b, Variant &v, bool isolated) { // the output record, and what `call` keeps per allele and genotype slot beside the device's arrays
            const uint64_t A = (uint64_t)v.n_alleles();
            recs.push_back({std::move(v.text_prefix), (uint32_t)A, isolated, b.n(), b.var_allele_off.back(), b.var_gt_off.back()});
            for (uint32_t a = 0; a < A; ++a) {
                b.freq.push_back(v.frequencies[a]);
                if (r.want_sample) b.allele_class.push_back(a ? allele_class_of(v.ref_sub, v.allele((int)a)) : (uint8_t)0);
            }
            b.var_gt_off.push_back(b.var_gt_off.back() + (r.haploid ? A : A * (A + 1) / 2));
        };
        // Every block takes the resident record loop (mg_cover_blocks: tier 1 for the lone records, tiers 2 and 3 for the others: the kernels bench.py
        // times).  MALVA_GENO_ISO_PATH=1 keeps the older split, where a lone record goes through the fused mg_call_isolated with a presence mask made
        // here (tests run both: same bytes) -- unless its right flank would cross the contig end: the device enumerator hands clipped windows to the host.
        // (k beyond the packed forms: exact-map keys live in the context's host-side list, which only the ASCII batch lookups reach)
        const bool lone_fits = r.k <= MG_MAX_PACKED_K && vb.is_lone_short() && base_found && right_flank_fits(vb.vars[0], r.k, reference.size());
        if (r.iso_path && lone_fits) {
            add_rec(iso, vb.vars[0], true);
            iso.LoneArrays::add(vb.vars[0], base_value, r.k, reference.size(), r.haploid);
        } else {
            // main.cpp:556-557: extract_kmers + set_coverages happen on the device for the whole batch of blocks.  A record of more than 127 alleles sends
            // its whole batch to the host enumerator (wide_alleles), which needs every record kept: its block is a batch of its own.  The records in front
            // of it, the lone ones a small panel has let go of among them, leave first; the batch is closed again behind it, so that no other block follows.
            bool wide = false;
            for (const Variant &v : vb.vars) wide = wide || v.n_alleles() > 127;
            if (wide && !recs.empty()) flush();
            if (wide) gen.wide_alleles = true;
            gen.open_block(base_value, reference.size());
            // a record tier 1 is sure to take (the device's own test, block_pipeline.h: classify_lone) can never be handed back:
            // with its genotype words made here, nothing of it needs keeping
            const bool sure_lone = gen.dense_gt && !gen.wide_alleles && !r.host_enum && lone_fits && vb.vars[0].ref_pos >= (int)r.k / 2;
            for (Variant &v : vb.vars) {
                add_rec(gen, v, false);
                gen.BlockArrays::add(v);
                gen.genotype_cells += v.n_genotypes();
                if (gen.dense_gt) { // one row of n_samples words per record (a record whose genotypes were not read -- it carries nothing -- keeps a row of zeros)
                    const size_t have = std::min(v.genotypes.size(), r.n_samples_kept);
                    for (size_t s_ = 0; s_ < have; ++s_) gen.gt_dense.push_back(genotype_word(v, s_, r.haploid));
                    gen.gt_dense.resize(gen.gt_dense.size() + (r.n_samples_kept - have), 0);
                }
                gen.var_slot.push_back(sure_lone ? -1 : (int32_t)gen.vars.size());
                if (!sure_lone) gen.vars.push_back(std::move(v)); // (the caller clears the block: its vector is used again)
            }
            gen.close_block();
            gen.block_ref.push_back(&reference);
            if (wide) flush();
        }
        if (gen.genotype_cells >= r.cell_bound) flush();
        if (recs.size() >= r.batch_records) flush();
    }
};

} // namespace malva
