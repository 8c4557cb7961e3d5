// The host-only slice of `index` and `call` between the record loop and the device (malva_amd/host/panel_batch.hpp) and behind it
// (malva_amd/host/call_text.hpp), driven without a device: the flat arrays of general blocks and of lone records, which records a
// batch of `call` keeps and when it closes, the panel's genotype words, the signature rows of a block the host enumerated, and the
// text and BCF records made from hand-written result arrays.  Every expected value is written out here; the text follows the
// reference's output_variants (var_block.hpp:337-396).  Meant to be built with -fsanitize=address,undefined and run on the CPU
// (`make sanitize-host`); tests/test_call_batch_cpu.py builds it plain.  Exits non-zero on the first wrong answer.
#define HOST_CHECK_NAME "call_batch_host_check"
#include "host_check_util.hpp"

#include "call_text.hpp"

using namespace malva;

//                                  k  haploid dense samples iso    host   sample records
static const BatchRules plain_rules{35, false, false, 2, false, false, false, 1000};

// ---- the eleven arrays of general blocks ------------------------------------------------------------------------------------------------
static std::vector<Block> two_blocks()
{
    Variant absent = var("c2", 70, "T", {"C", "C"});
    absent.is_present = false;
    std::vector<Block> b;
    b.push_back(block_of(35, {var("c1", 50, "A", {"G"})}));
    b.push_back(block_of(35, {var("c2", 60, "AC", {"A", "ACGT"}), absent}));
    return b;
}
static void check_block_fields(const BlockArrays &a)
{
    CHECK(a.n() == 3 && a.n_blocks() == 2 && !a.wide_alleles);
    CHECK(same<uint64_t>(a.blk_base, {100, 1100}));
    CHECK(same<uint32_t>(a.blk_len, {1000, 500}));
    CHECK(same<uint32_t>(a.blk_var_off, {0, 1, 3}));
    CHECK(same<int32_t>(a.ipos, {50, 60, 70}));
    CHECK(same<uint32_t>(a.ref_size, {1, 2, 1}));
    CHECK(same<uint32_t>(a.min_size, {1, 1, 1}));
    CHECK(same<uint8_t>(a.is_present, {1, 1, 0}));
    CHECK(same<uint32_t>(a.var_allele_off, {0, 2, 5, 8}));
    CHECK(same<uint32_t>(a.allele_off, {0, 1, 2, 4, 5, 9, 10, 11, 12}));
    CHECK(std::string(a.pool.begin(), a.pool.end()) == "AG" "ACAACGT" "TCC");
    CHECK(same<uint8_t>(a.canon, {0, 1, 0, 1, 2, 0, 1, 1})); // (the second C of the last record is its first)
    CHECK(a.blk_var_off.back() == a.n() && a.var_allele_off.back() == a.canon.size() && a.allele_off.back() == a.pool.size());
}
static void check_block_arrays()
{
    BlockArrays index_side; // as index_main's enumerate_waiting fills one
    const std::vector<Block> waiting = two_blocks();
    const uint64_t base[2] = {100, 1100};
    const size_t len[2] = {1000, 500};
    for (size_t b = 0; b < 2; ++b) {
        index_side.open_block(base[b], len[b]);
        for (const Variant &v : waiting[b].vars) index_side.add(v);
        index_side.close_block();
    }
    check_block_fields(index_side);

    Pass call_side(plain_rules); // as call_main's record loop fills one
    std::vector<Block> blocks = two_blocks();
    call_side.add(std::move(blocks[0]));
    call_side.add(std::move(blocks[1]), "c2");
    CHECK(call_side.closed.empty());
    call_side.b.flush();
    CHECK(call_side.closed.size() == 1);
    const Batch &gen = call_side.closed[0].gen;
    check_block_fields(gen);
    CHECK(gen.n() == 3 && gen.pos.empty() && call_side.closed[0].iso.n() == 0);
    // what `call` keeps on top: frequencies per allele slot, genotype slots (diploid: A (A + 1) / 2), the records, their contigs
    CHECK(same<float>(gen.freq, {0.5f, 0.25f, 0.5f, 0.25f, 0.125f, 0.5f, 0.25f, 0.125f}));
    CHECK(same<uint64_t>(gen.var_gt_off, {0, 3, 9, 15}) && gen.allele_class.empty());
    CHECK(same<int32_t>(gen.var_slot, {0, 1, 2}) && gen.vars.size() == 3 && gen.vars[1].ref_sub == "AC");
    CHECK(gen.block_ref.size() == 2 && gen.block_ref[0] == &call_side.ref1 && gen.block_ref[1] == &call_side.ref2);
    CHECK(gen.genotype_cells == 6 && gen.gt_dense.empty());
    const std::vector<Rec> &recs = call_side.closed[0].recs;
    CHECK(recs.size() == 3 && recs[0].prefix == "c1\t51\t.\tA\tG\t." && recs[2].prefix == "c2\t71\t.\tT\tC,C\t.");
    CHECK(recs[1].n_alleles == 3 && !recs[1].isolated && recs[1].slot == 1 && recs[1].allele0 == 2 && recs[1].gt0 == 3);
    CHECK(recs[2].n_alleles == 3 && recs[2].slot == 2 && recs[2].allele0 == 5 && recs[2].gt0 == 9);

    // haploid: one genotype slot per allele; --sample-stats: the alleles' classes (REF: 0; AC > A: deletion; AC > ACGT: insertion)
    BatchRules rules = plain_rules;
    rules.haploid = rules.want_sample = true;
    Pass with_classes(rules);
    blocks = two_blocks();
    with_classes.add(std::move(blocks[0]));
    with_classes.add(std::move(blocks[1]), "c2");
    CHECK(same<uint64_t>(with_classes.b.gen.var_gt_off, {0, 2, 5, 8}));
    CHECK(same<uint8_t>(with_classes.b.gen.allele_class, {0, 1, 0, 4, 3, 0, 1, 1}));

    // 127 alleles fit the device's 7-bit allele numbers, 128 do not
    for (int n_alts : {126, 127}) {
        BlockArrays a;
        a.open_block(0, 1000);
        a.add(var("c1", 50, "A", std::vector<std::string>((size_t)n_alts, "G")));
        a.close_block();
        CHECK(a.wide_alleles == (n_alts == 127) && a.var_allele_off.back() == (uint32_t)n_alts + 1);
    }
}

// ---- the six arrays of lone records, the flank --------------------------------------------------------------------------------------------
static void check_lone_arrays()
{
    for (int k : {35, 31}) {
        const int len = 200;
        Variant absent = var("c1", 100, "A", {"G"});
        absent.is_present = false;
        LoneArrays a;
        // every sample 0|1: both alleles are carried where the record is eligible (var_block.hpp:104: k <= pos <= len - k)
        for (int pos : {k - 1, k, len - k, len - k + 1, -1}) a.add(var("c1", pos, "A", {"G"}), 1000, (unsigned)k, (size_t)len, false);
        a.add(absent, 1000, (unsigned)k, (size_t)len, false);
        a.add(var("c1", 100, "AT", {"A", "ATT"}, 2, 2, 0), 1000, (unsigned)k, (size_t)len, false); // 2|0: alleles 2 and 0
        a.add(var("c1", 100, "AT", {"A", "ATT"}, 2, 2, 1), 1000, (unsigned)k, (size_t)len, true);  // haploid: the first alone
        CHECK(a.n() == 8);
        CHECK(same<uint8_t>(a.flags, {0, 1, 1, 0, 0, 0, 1, 1}));
        CHECK(same<uint64_t>(a.present, {0, 3, 3, 0, 0, 0, 5, 4}));
        CHECK(same<uint64_t>(a.pos, {1000 + (uint64_t)k - 1, 1000 + (uint64_t)k, 1200 - (uint64_t)k, 1201 - (uint64_t)k, 1000, 1100, 1100, 1100}));
        CHECK(same<uint32_t>(a.var_allele_off, {0, 2, 4, 6, 8, 10, 12, 15, 18}));
        CHECK(std::string(a.pool.begin(), a.pool.end()) == "AGAGAGAGAGAG" "ATAATT" "ATAATT");
        CHECK(same<uint32_t>(a.allele_off, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 18, 20, 21, 24}));
        CHECK(a.allele_off.back() == a.pool.size());

        // the right flank: ceil(k / 2) bases behind the REF allele -- 18 for k = 35, 16 for k = 31
        const int half_up = k == 35 ? 18 : 16;
        const Variant del = var("c1", 100, "AT", {"A"});
        CHECK(right_flank_fits(del, (unsigned)k, (size_t)(100 + 2 + half_up)));
        CHECK(!right_flank_fits(del, (unsigned)k, (size_t)(100 + 2 + half_up - 1)));
    }
}

// ---- which records a batch keeps -------------------------------------------------------------------------------------------------------------
static void check_kept_records()
{
    BatchRules dense = plain_rules;
    dense.dense_gt = true;
    auto cluster = [] { return block_of(35, {var("c1", 200, "A", {"G"}, 2, 1, 1), var("c1", 210, "C", {"T"}, 2, 0, 0, false)}); };
    {
        Pass p(dense); // a sure-lone record is let go of, a clustered one kept
        p.add(block_of(35, {var("c1", 100, "A", {"G"})}));
        p.add(cluster());
        const Batch &g = p.b.gen;
        CHECK(same<int32_t>(g.var_slot, {-1, 0, 1}) && g.vars.size() == 2 && g.vars[0].ref_pos == 200 && g.vars[1].ref_pos == 210);
        // its genotype words were made here: a1 | a2 << 7 | phased << 14, a row of two samples per record
        CHECK(same<uint16_t>(g.gt_dense, {0x4080, 0x4080, 0x4081, 0x4081, 0, 0}));
        CHECK(p.b.recs.size() == 3 && same<uint32_t>(g.blk_var_off, {0, 1, 3}));
    }
    {
        BatchRules r = dense; // the host enumerator takes every block: every record is kept for it
        r.host_enum = true;
        Pass p(r);
        p.add(block_of(35, {var("c1", 100, "A", {"G"})}));
        p.add(cluster());
        CHECK(same<int32_t>(p.b.gen.var_slot, {0, 1, 2}) && p.b.gen.vars.size() == 3);
    }
    {
        Pass p(plain_rules); // no words made while batching: the worker packs them from the records
        p.add(block_of(35, {var("c1", 100, "A", {"G"})}));
        CHECK(same<int32_t>(p.b.gen.var_slot, {0}) && p.b.gen.vars.size() == 1 && p.b.gen.gt_dense.empty());
    }
    {
        Pass p(dense); // tier 1's own test: pos >= k / 2 (17), and the right flank inside the contig (pos + 1 + 18 <= 1000)
        for (int pos : {16, 17, 981, 982}) p.add(block_of(35, {var("c1", pos, "A", {"G"})}));
        p.add(block_of(35, {var("c9", 100, "A", {"G"})}), "c9"); // (a contig the device does not hold)
        CHECK(same<int32_t>(p.b.gen.var_slot, {0, -1, -1, 1, 2}));
        CHECK(same<uint64_t>(p.b.gen.blk_base, {100, 100, 100, 100, 0}));
    }
    {
        BatchRules r = dense; // k beyond the packed forms: nothing is let go of
        r.k = 65;
        Pass p(r);
        p.add(block_of(65, {var("c1", 100, "A", {"G"})}));
        CHECK(same<int32_t>(p.b.gen.var_slot, {0}));
    }
    {
        // A batch that goes to the host enumerator as a whole needs every record, the lone ones behind a wide record too.  No sequence of add_block
        // calls leaves a record behind a wide one -- a wide block is closed behind itself --, so the flag is set by hand: this pins sure_lone's own term
        Pass p(dense);
        p.b.gen.wide_alleles = true;
        p.add(block_of(35, {var("c1", 100, "A", {"G"})}));
        CHECK(same<int32_t>(p.b.gen.var_slot, {0}) && p.b.gen.vars.size() == 1);
    }
}

// ---- when a batch closes ---------------------------------------------------------------------------------------------------------------------
static void check_closes()
{
    BatchRules dense = plain_rules;
    dense.dense_gt = true;
    auto lone = [](int pos) { return block_of(35, {var("c1", pos, "A", {"G"})}); };
    auto fresh = [](const Pass &p) {
        const Batch &g = p.b.gen, &i = p.b.iso;
        return p.b.recs.empty() && g.dense_gt && !i.dense_gt && !g.wide_alleles && g.n() == 0 && i.n() == 0 && same<uint32_t>(g.blk_var_off, {0}) &&
               same<uint32_t>(g.var_allele_off, {0}) && same<uint32_t>(g.allele_off, {0}) && same<uint64_t>(g.var_gt_off, {0}) &&
               same<uint32_t>(i.var_allele_off, {0}) && same<uint32_t>(i.allele_off, {0}) && same<uint64_t>(i.var_gt_off, {0}) && g.pool.empty() &&
               g.vars.empty() && g.var_slot.empty() && g.gt_dense.empty() && g.block_ref.empty() && g.genotype_cells == 0;
    };
    {
        Pass p(dense); // a wide block: the records in front of it leave first, it leaves alone
        p.add(lone(100));
        p.add(lone(300));
        CHECK(p.closed.empty());
        p.add(block_of(35, {var("c1", 500, "A", std::vector<std::string>(127, "G")), var("c1", 505, "C", {"T"})}));
        CHECK(p.closed.size() == 2 && fresh(p));
        CHECK(p.closed[0].recs.size() == 2 && !p.closed[0].gen.wide_alleles && same<int32_t>(p.closed[0].gen.var_slot, {-1, -1}));
        const Batch &wide = p.closed[1].gen;
        CHECK(p.closed[1].recs.size() == 2 && wide.wide_alleles && wide.n_blocks() == 1 && same<int32_t>(wide.var_slot, {0, 1}) && wide.vars.size() == 2);
        p.add(lone(700));
        p.b.flush();
        CHECK(p.closed.size() == 3 && p.closed[2].recs.size() == 1 && !p.closed[2].gen.wide_alleles && same<int32_t>(p.closed[2].gen.var_slot, {-1}) && fresh(p));
    }
    {
        Pass p(dense); // a wide block at the head of a pass: no empty batch in front of it
        p.add(block_of(35, {var("c1", 500, "A", std::vector<std::string>(127, "G"))}));
        CHECK(p.closed.size() == 1 && p.closed[0].recs.size() == 1 && fresh(p));
    }
    {
        BatchRules r = dense; // the record count: when the third record lands, not before
        r.batch_records = 3;
        Pass p(r);
        p.add(lone(100));
        p.add(lone(300));
        CHECK(p.closed.empty() && p.b.recs.size() == 2);
        p.add(lone(500));
        CHECK(p.closed.size() == 1 && p.closed[0].recs.size() == 3 && p.closed[0].gen.n() == 3 && fresh(p));
        p.add(block_of(35, {var("c1", 600, "A", {"G"}), var("c1", 601, "C", {"T"}), var("c1", 602, "G", {"T"}), var("c1", 603, "T", {"A"})})); // (a block is never split)
        CHECK(p.closed.size() == 2 && p.closed[1].recs.size() == 4 && fresh(p));
    }
    {
        BatchRules r = dense; // the genotype cells, two per record here: the close follows the record that reaches the bound
        r.cell_bound = 5;
        Pass p(r);
        p.add(lone(100));
        p.add(lone(300));
        CHECK(p.closed.empty() && p.b.gen.genotype_cells == 4);
        p.add(lone(500));
        CHECK(p.closed.size() == 1 && p.closed[0].gen.genotype_cells == 6 && p.closed[0].recs.size() == 3 && fresh(p));
    }
    {
        BatchRules r = dense; // MALVA_GENO_ISO_PATH: a lone record whose flank fits goes to the batch of mg_call_isolated, with its mask
        r.iso_path = true;
        Pass p(r);
        p.add(lone(100));
        p.add(lone(982)); // (the flank does not fit: the general batch, kept)
        p.add(lone(300));
        const Batch &i = p.b.iso;
        CHECK(i.n_blocks() == 0 && i.n() == 2 && same<uint64_t>(i.pos, {200, 400}) && same<uint64_t>(i.present, {3, 3}) && same<uint8_t>(i.flags, {1, 1}));
        CHECK(same<uint64_t>(i.var_gt_off, {0, 3, 6}) && same<float>(i.freq, {0.5f, 0.25f, 0.5f, 0.25f}) && p.b.gen.n() == 1 && same<int32_t>(p.b.gen.var_slot, {0}));
        CHECK(p.b.recs.size() == 3 && p.b.recs[0].isolated && !p.b.recs[1].isolated && p.b.recs[2].isolated);
        CHECK(p.b.recs[2].slot == 1 && p.b.recs[2].allele0 == 2 && p.b.recs[2].gt0 == 3 && p.b.recs[1].slot == 0);
    }
}

// ---- the panel's genotype words ----------------------------------------------------------------------------------------------------------------
static void check_genotypes()
{
    Variant v = var("c1", 100, "A", {"G"}, 3, 1, 0, false);
    CHECK(genotype_word(v, 0, false) == 1 && genotype_word(v, 0, true) == 0x4001);
    v.genotypes[1] = {0, 1};
    v.phasing[1] = 1;
    CHECK(genotype_word(v, 1, false) == 0x4080);
    v.genotypes[2] = {2, 0}; // an allele number equal to n_alleles()
    CHECK(throws([&] { genotype_word(v, 2, false); }));
    v.genotypes[2] = {0, 2};
    CHECK(throws([&] { genotype_word(v, 2, false); }));

    for (size_t n : {64, 65}) { // 64 samples: the dense matrix; 65: per record the samples that differ from the default word
        std::vector<Variant> recs{var("c1", 100, "A", {"G"}, n, 0, 0), var("c1", 200, "A", {"G"}, n, 0, 0)};
        recs[1].genotypes[3] = {1, 0};
        recs[1].phasing[3] = 0;
        const PanelGenotypes g = pack_genotypes(recs, 2, (uint32_t)n, false);
        CHECK(g.sparse == (n == 65));
        if (n == 64) {
            CHECK(g.gt.size() == 128 && g.gt[0] == 0x4000 && g.gt[63] == 0x4000 && g.gt[64 + 3] == 1 && g.gt[64 + 4] == 0x4000 && g.bytes() == 256);
        } else {
            CHECK(g.gt.empty() && g.sp_default == 0x4000 && same<uint32_t>(g.sp_off, {0, 0, 1}) && same<uint32_t>(g.sp_sample, {3}) && same<uint16_t>(g.sp_gt, {1}));
        }
    }
    { // the default word follows the majority: a panel of 0/0 takes 0, and its one phased sample becomes the entry
        std::vector<Variant> recs{var("c1", 100, "A", {"G"}, 65, 0, 0, false)};
        recs[0].phasing[7] = 1;
        const PanelGenotypes g = pack_genotypes(recs, 1, 65, false);
        CHECK(g.sparse && g.sp_default == 0 && same<uint32_t>(g.sp_off, {0, 1}) && same<uint32_t>(g.sp_sample, {7}) && same<uint16_t>(g.sp_gt, {0x4000}));
    }
    { // records decoded on the device arrive sparse against their own batch's default: two of 0/0 outvote one of 0|0, which is re-expressed
        auto deferred = [](uint16_t dflt) {
            Variant d = var("c1", 100, "A", {"G"}, 0);
            d.gt_deferred = true;
            d.n_kept = 3;
            d.max_allele = 1;
            d.sp_default = dflt;
            return d;
        };
        std::vector<Variant> recs{deferred(0), deferred(0), deferred(0x4000)};
        recs[1].sp_sample = {2};
        recs[1].sp_gt = {0x0081};
        recs[2].sp_sample = {1};
        recs[2].sp_gt = {0x4081};
        const PanelGenotypes g = pack_genotypes(recs, 3, 3, false);
        CHECK(g.sparse && g.sp_default == 0 && same<uint32_t>(g.sp_off, {0, 0, 1, 4}));
        CHECK(same<uint32_t>(g.sp_sample, {2, 0, 1, 2}) && same<uint16_t>(g.sp_gt, {0x0081, 0x4000, 0x4081, 0x4000}));
        recs[0].max_allele = 2; // an allele number equal to n_alleles()
        CHECK(throws([&] { pack_genotypes(recs, 3, 3, false); }));
    }
    { // the blocks of the index side give the same words as their records in a row
        std::vector<Block> blocks;
        blocks.push_back(block_of(35, {var("c1", 100, "A", {"G"}, 2, 1, 1)}));
        blocks.push_back(block_of(35, {var("c1", 200, "A", {"G"}, 2, 0, 1), var("c1", 210, "C", {"T"}, 2, 0, 0, false)}));
        CHECK(same<uint16_t>(pack_genotypes(blocks, 3, 2, false).gt, {0x4081, 0x4081, 0x4080, 0x4080, 0, 0}));
        CHECK(same<uint16_t>(pack_genotypes(blocks, 3, 2, true).gt, {0x4001, 0x4001, 0x4000, 0x4000, 0x4000, 0x4000}));
    }
}

static void check_allele_class()
{
    CHECK(allele_class_of("A", "G") == 1 && allele_class_of("G", "A") == 1 && allele_class_of("C", "T") == 1 && allele_class_of("T", "C") == 1);
    CHECK(allele_class_of("A", "C") == 2 && allele_class_of("A", "T") == 2 && allele_class_of("G", "C") == 2 && allele_class_of("G", "T") == 2);
    CHECK(allele_class_of("A", "AT") == 3 && allele_class_of("AT", "A") == 4 && allele_class_of("ACG", "AT") == 4);
    CHECK(allele_class_of("A", "*") == 5 && allele_class_of("A", "<DEL>") == 5 && allele_class_of("A", "N") == 5 && allele_class_of("AC", "ANC") == 5);
    CHECK(allele_class_of("AC", "GT") == 5);
    CHECK(allele_class_of("a", "g") == 1 && allele_class_of("a", "C") == 2 && allele_class_of("a", "at") == 3 && allele_class_of("at", "a") == 4);
}

// ---- the signatures of a block the host enumerated --------------------------------------------------------------------------------------------
static void check_signature_rows()
{
    const Block blk = block_of(35, {var("c1", 100, "A", {"G"}), var("c1", 110, "C", {"T"})});
    std::vector<AlleleSignatures> sigs(2);
    sigs[0][0] = {{"ACGT", "CGTA"}};  // REF of the first record: one signature of two k-mers; its ALT has none
    sigs[1][1] = {{"GGGG"}, {"TTTT"}}; // ALT of the second: two signatures of one
    const SignatureRows s = signature_rows(blk, sigs);
    CHECK(s.rows.n == 4 && s.rows.data.size() == 4 * STRIDE);
    const char *want[4] = {"ACGT", "CGTA", "GGGG", "TTTT"};
    for (size_t i = 0; i < 4; ++i) {
        CHECK(std::string(&s.rows.data[i * STRIDE]) == want[i]);
        for (size_t j = 4; j < STRIDE; ++j) CHECK(s.rows.data[i * STRIDE + j] == 0);
    }
    CHECK(same<uint8_t>(s.is_ref, {1, 1, 0, 0}));
    CHECK(same<uint64_t>(s.sig_off, {0, 2, 3, 4}));
    CHECK(same<uint64_t>(s.al_off, {0, 1, 1, 1, 3})); // (an allele without signatures still has its slot)
    sigs[1][1][1][0] = std::string(MG_MAX_KMER, 'A');
    CHECK(signature_rows(blk, sigs).rows.n == 4);
    sigs[1][1][1][0] = std::string(MG_MAX_KMER + 1, 'A');
    CHECK(throws([&] { signature_rows(blk, sigs); }));
}

// ---- the per-sample lines ------------------------------------------------------------------------------------------------------------------------
// One lone record (two alleles) and two others (two and three alleles), interleaved; two planes whose values differ everywhere.
struct Results {
    std::vector<Rec> recs;
    Batch iso, gen;
};
static Results results(bool haploid)
{
    Results r;
    r.iso.var_allele_off = {0, 2};
    r.gen.var_allele_off = {0, 2, 5};
    r.recs = {{"c1\t101\t.\tA\tG\t.", 2, false, 0, 0, 0}, {"c1\t301\trs1\tC\tT\t50", 2, true, 0, 0, 0}, {"c2\t7\t.\tAC\tA,ACGT\t.", 3, false, 1, 2, haploid ? 2u : 3u}};
    const double nan = std::nan("");
    //               plane 0                          plane 1
    r.iso.cov = {7, 8, /**/ 0, 9};
    r.iso.status = {MG_GT_SINGLE, /**/ MG_GT_NOCOV};
    r.iso.g1 = {0, /**/ 0};
    r.iso.g2 = {0, /**/ 0};
    r.iso.gq = {100, /**/ 0};
    r.iso.probs.assign(haploid ? 4 : 6, 0.125); // (never read: neither plane's status is normal)
    r.gen.cov = {3, 4, 201, 5, 300, /**/ 30, 40, 1, 200, 2};
    r.gen.status = {MG_GT_NORMAL, MG_GT_OVERCOV, /**/ MG_GT_NORMAL, MG_GT_NORMAL};
    r.gen.g1 = {0, 0, /**/ 1, 0};
    r.gen.g2 = {1, 0, /**/ 1, 2};
    r.gen.gq = {57, 0, /**/ 99, 42};
    if (haploid) r.gen.probs = {0.5, nan, 9, 9, 9, /**/ 0.25, 0.75, 0.1, 0.2, 0.7};
    else r.gen.probs = {0.5, nan, 0.25, 9, 9, 9, 9, 9, 9, /**/ 0, 0.000001, 0.999999, 0.1, 0.2, 0.3, 0.4, 0.0000004, 1};
    return r;
}
static void check_per_sample_lines()
{
    auto lines = [](bool haploid, bool verbose, size_t pl) {
        const Results r = results(haploid);
        std::vector<std::string> outs{"#", "#"}; // (appended to: what a plane's string holds stays)
        per_sample_lines(outs, r.recs, r.iso, r.gen, 2, haploid, verbose, 200);
        return outs[pl];
    };
    CHECK(lines(false, false, 0) == "#c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t0/1:57\n"
                                    "c1\t301\trs1\tC\tT\t50\tPASS\t.\tGT:GQ\t0/0:100\n"
                                    "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\t.\tGT:GQ\t0/0:0\n");
    CHECK(lines(false, false, 1) == "#c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1/1:99\n"
                                    "c1\t301\trs1\tC\tT\t50\tPASS\t.\tGT:GQ\t0/0:0\n"
                                    "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\t.\tGT:GQ\t0/2:42\n");
    // -v, plane 0: a NaN likelihood prints as the reference's -nan; one allele alone: 1.000000; two of three alleles over 200: two entries
    CHECK(lines(false, true, 0) == "#c1\t101\t.\tA\tG\t.\tPASS\tCOVS=3,4;GTS=0/0:0.500000,0/1:-nan,1/1:0.250000\tGT:GQ\t0/1:57\n"
                                   "c1\t301\trs1\tC\tT\t50\tPASS\tCOVS=7,8;GTS=0/0:1.000000\tGT:GQ\t0/0:100\n"
                                   "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\tCOVS=201,5,300;GTS=0/0:-nan,0/0:-nan\tGT:GQ\t0/0:0\n");
    // plane 1 reads pl * bn + slot, pl * bna + allele0, pl * bng + gt0; a coverage AT the limit is not over it; no coverage: one -nan entry
    CHECK(lines(false, true, 1) == "#c1\t101\t.\tA\tG\t.\tPASS\tCOVS=30,40;GTS=0/0:0.000000,0/1:0.000001,1/1:0.999999\tGT:GQ\t1/1:99\n"
                                   "c1\t301\trs1\tC\tT\t50\tPASS\tCOVS=0,9;GTS=0/0:-nan\tGT:GQ\t0/0:0\n"
                                   "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\tCOVS=1,200,2;GTS=0/0:0.100000,0/1:0.200000,0/2:0.300000,1/1:0.400000,1/2:0.000000,2/2:1.000000\tGT:GQ\t0/2:42\n");
    CHECK(lines(true, false, 1) == "#c1\t101\t.\tA\tG\t.\tPASS\t.\tGT:GQ\t1:99\n"
                                   "c1\t301\trs1\tC\tT\t50\tPASS\t.\tGT:GQ\t0:0\n"
                                   "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\t.\tGT:GQ\t0:42\n");
    CHECK(lines(true, true, 0) == "#c1\t101\t.\tA\tG\t.\tPASS\tCOVS=3,4;GTS=0:0.500000,1:-nan\tGT:GQ\t0:57\n"
                                  "c1\t301\trs1\tC\tT\t50\tPASS\tCOVS=7,8;GTS=0:1.000000\tGT:GQ\t0:100\n"
                                  "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\tCOVS=201,5,300;GTS=0:-nan,0:-nan\tGT:GQ\t0:0\n");
    CHECK(lines(true, true, 1) == "#c1\t101\t.\tA\tG\t.\tPASS\tCOVS=30,40;GTS=0:0.250000,1:0.750000\tGT:GQ\t1:99\n"
                                  "c1\t301\trs1\tC\tT\t50\tPASS\tCOVS=0,9;GTS=0:-nan\tGT:GQ\t0:0\n"
                                  "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\tCOVS=1,200,2;GTS=0:0.100000,1:0.200000,2:0.700000\tGT:GQ\t0:42\n");
}

// ---- the merged output -------------------------------------------------------------------------------------------------------------------------
struct MergedRows { // as `process` holds them: [0] the lone records', [1] the others'
    std::vector<char> row_text[2], info_text[2];
    std::vector<uint64_t> row_off[2], info_off[2];
    std::vector<uint32_t> site_ac[2], site_ns[2];
};
static MergedRows merged_rows()
{
    MergedRows m; // the lone record's row and INFO in [0], the two others' in [1]
    const std::string lone_row = "\t0/0:100\t0/0:0\n", rows = "\t0/1:57\t1/1:99\n" "\t0/0:0\t0/2:42\n";
    m.row_text[0].assign(lone_row.begin(), lone_row.end());
    m.row_off[0] = {0, 15};
    m.row_text[1].assign(rows.begin(), rows.end());
    m.row_off[1] = {0, 15, 29};
    const std::string lone_info = "AC=0;AN=2;AF=0;NS=1", infos = "AC=3;AN=4;AF=0.75;NS=2" "AC=0,1;AN=2;AF=0,0.5;NS=1";
    m.info_text[0].assign(lone_info.begin(), lone_info.end());
    m.info_off[0] = {0, 19};
    m.info_text[1].assign(infos.begin(), infos.end());
    m.info_off[1] = {0, 22, 47};
    m.site_ac[0] = {2, 0};
    m.site_ns[0] = {1};
    m.site_ac[1] = {1, 3, 1, 0, 1};
    m.site_ns[1] = {2, 1};
    return m;
}
static void check_merged_text()
{
    const Results r = results(false);
    const MergedRows m = merged_rows();
    const char *formats[2][2] = {{"GT:GQ", "GT:GQ:GP"}, {"GT:GQ:COVS", "GT:GQ:COVS:GP"}};
    for (int verbose = 0; verbose < 2; ++verbose)
        for (int gp = 0; gp < 2; ++gp) {
            const std::string f = formats[verbose][gp];
            std::string out = "#";
            merged_text_lines(out, r.recs, m.row_text, m.row_off, m.info_text, m.info_off, verbose, gp, true, false); // the first group's block, INFO left to the paste pass (or no --site-tags)
            CHECK(out == "#c1\t101\t.\tA\tG\t.\tPASS\t.\t" + f + "\t0/1:57\t1/1:99\n" +
                             "c1\t301\trs1\tC\tT\t50\tPASS\t.\t" + f + "\t0/0:100\t0/0:0\n" +
                             "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\t.\t" + f + "\t0/0:0\t0/2:42\n");
            out = "#";
            merged_text_lines(out, r.recs, m.row_text, m.row_off, m.info_text, m.info_off, verbose, gp, true, true); // one group with --site-tags: INFO made at once
            CHECK(out == "#c1\t101\t.\tA\tG\t.\tPASS\tAC=3;AN=4;AF=0.75;NS=2\t" + f + "\t0/1:57\t1/1:99\n" +
                             "c1\t301\trs1\tC\tT\t50\tPASS\tAC=0;AN=2;AF=0;NS=1\t" + f + "\t0/0:100\t0/0:0\n" +
                             "c2\t7\t.\tAC\tA,ACGT\t.\tPASS\tAC=0,1;AN=2;AF=0,0.5;NS=1\t" + f + "\t0/0:0\t0/2:42\n");
            for (int info_here = 0; info_here < 2; ++info_here) { // a later group: its sample columns alone
                out = "#";
                merged_text_lines(out, r.recs, m.row_text, m.row_off, m.info_text, m.info_off, verbose, gp, false, info_here);
                CHECK(out == "#\t0/1:57\t1/1:99\n" "\t0/0:100\t0/0:0\n" "\t0/0:0\t0/2:42\n");
            }
        }
}

static uint32_t u32_at(const std::string &s, size_t at)
{
    CHECK(at + 4 <= s.size());
    uint32_t v;
    memcpy(&v, &s[at], 4);
    return v;
}
static std::string inflate_bgzf(const std::string &bytes)
{
    std::string plain;
    for (size_t at = 0; at < bytes.size();) {
        CHECK(at + 18 <= bytes.size() && (unsigned char)bytes[at] == 0x1f && (unsigned char)bytes[at + 1] == 0x8b && bytes[at + 12] == 'B' && bytes[at + 13] == 'C');
        const size_t size = ((unsigned char)bytes[at + 16] | (size_t)(unsigned char)bytes[at + 17] << 8) + 1;
        CHECK(size >= 26 && at + size <= bytes.size());
        const uint32_t isize = u32_at(bytes, at + size - 4);
        std::string piece((size_t)isize + 1, '\0');
        z_stream zs{};
        CHECK(inflateInit2(&zs, -15) == Z_OK);
        zs.next_in = (Bytef *)&bytes[at + 18];
        zs.avail_in = (uInt)(size - 26);
        zs.next_out = (Bytef *)&piece[0];
        zs.avail_out = isize + 1;
        const int rc = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        CHECK(rc == Z_STREAM_END && zs.total_out == isize);
        plain.append(piece, 0, isize);
        at += size;
    }
    return plain;
}
static void check_merged_bcf()
{
    const Results r = results(false);
    const MergedRows m = merged_rows();
    const BcfHeader hdr = bcf_parse_header("##fileformat=VCFv4.2\n##contig=<ID=c1>\n##contig=<ID=c2>\n##INFO=<ID=AC,Number=A,Type=Integer>\n##INFO=<ID=AN,Number=1,Type=Integer>\n"
                                           "##INFO=<ID=AF,Number=A,Type=Float>\n##INFO=<ID=NS,Number=1,Type=Integer>\n##FORMAT=<ID=GT,Number=1,Type=String>\n"
                                           "##FORMAT=<ID=GQ,Number=1,Type=Integer>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n",
                                           true);
    // the shared block without INFO: 24 bytes of fixed fields, ID, REF, every ALT (a typed string: one byte and its text; '.': the byte alone), FILTER [PASS]
    const uint32_t want_shared[3] = {24 + 1 + 2 + 2 + 2, 24 + 4 + 2 + 2 + 2, 24 + 1 + 3 + 2 + 5 + 2}, want_chrom[3] = {0, 0, 1}, want_pos0[3] = {100, 300, 6}, want_alleles[3] = {2, 2, 3};
    const std::string want_row[3] = {"\t0/1:57\t1/1:99\n", "\t0/0:100\t0/0:0\n", "\t0/0:0\t0/2:42\n"};
    std::string direct_plain;
    for (int tags = 0; tags < 2; ++tags) { // one group: whole records
        std::string out = "#";
        merged_bcf_records(out, r.recs, m.row_text, m.row_off, m.site_ac, m.site_ns, hdr, 2, 2, true, true, tags, false);
        size_t at = 1;
        for (int i = 0; i < 3; ++i) {
            const uint32_t l_shared = u32_at(out, at), l_indiv = u32_at(out, at + 4);
            CHECK(l_indiv == want_row[i].size() && out.compare(at + 8 + l_shared, l_indiv, want_row[i]) == 0); // (they equal the lengths of what follows)
            if (!tags) CHECK(l_shared == want_shared[i]);
            else CHECK(l_shared > want_shared[i]);
            CHECK(u32_at(out, at + 8) == want_chrom[i] && u32_at(out, at + 12) == want_pos0[i]);
            CHECK(u32_at(out, at + 8 + 16) == (want_alleles[i] << 16 | (tags ? 4u : 0u))); // n_allele << 16 | n_info: AC, AN, AF, NS
            CHECK(u32_at(out, at + 8 + 20) == (2u << 24 | 2u));                            // n_fmt << 24 | n_sample
            CHECK(out[at + 8 + l_shared - 2] == 0x11 || tags);
            at += 8 + l_shared + l_indiv;
        }
        CHECK(at == out.size());
        if (!tags) direct_plain = out.substr(1);
    }
    {
        std::string out; // BGZF: the same bytes, compressed
        merged_bcf_records(out, r.recs, m.row_text, m.row_off, m.site_ac, m.site_ns, hdr, 2, 2, true, true, false, true);
        CHECK(!out.empty() && out != direct_plain && inflate_bgzf(out) == direct_plain);
    }
    for (int fixed = 0; fixed < 2; ++fixed) { // several groups: every piece behind its u32 length, the shared block in the first group's file alone
        std::string out = "#";
        merged_bcf_records(out, r.recs, m.row_text, m.row_off, m.site_ac, m.site_ns, hdr, 2, 2, fixed, false, true, true); // (no INFO and no compression here: the paste pass makes both)
        size_t at = 1;
        for (int i = 0; i < 3; ++i) {
            if (fixed) {
                CHECK(u32_at(out, at) == want_shared[i] && u32_at(out, at + 4) == want_chrom[i] && u32_at(out, at + 4 + 16) == want_alleles[i] << 16);
                CHECK(u32_at(out, at + 4 + 20) == 2u << 24); // (n_sample: the paste pass knows the cohort)
                at += 4 + want_shared[i];
            }
            CHECK(u32_at(out, at) == want_row[i].size() && out.compare(at + 4, want_row[i].size(), want_row[i]) == 0);
            at += 4 + want_row[i].size();
        }
        CHECK(at == out.size());
    }
}

static void check_small_things()
{
    Reference refs;
    refs.names = {"c2", "c1"}; // (FASTA order, not name order)
    refs.seqs["c1"] = "ACGT";
    refs.seqs["c2"] = "GG";
    std::map<std::string, uint64_t> base;
    CHECK(concat_reference(refs, base) == "GGACGT" && base.size() == 2 && base["c2"] == 0 && base["c1"] == 2);
    unsetenv("MALVA_GENO_BATCH");
    CHECK(geno_batch_records(200000) == 200000 && geno_batch_records(65536) == 65536);
    setenv("MALVA_GENO_BATCH", "7", 1);
    CHECK(geno_batch_records(200000) == 7);
    setenv("MALVA_GENO_BATCH", "0", 1);
    CHECK(geno_batch_records(200000) == 1);
    unsetenv("MALVA_GENO_BATCH");
}

int main()
{
    check_block_arrays();
    check_lone_arrays();
    check_kept_records();
    check_closes();
    check_genotypes();
    check_allele_class();
    check_signature_rows();
    check_per_sample_lines();
    check_merged_text();
    check_merged_bcf();
    check_small_things();
    std::cout << "call_batch_host_check: ok\n";
    return 0;
}
